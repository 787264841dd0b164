"""Host logic on the CPU: the product front end must build the reference's table exactly (checked against the
oracle row by row), and both device programs must keep its language (replayed in Python).  No GPU needed."""
import random

import numpy as np

import pytest

import roaringregex_amd as rr
from patterns import EMAIL, K1000, K1000_CONTAINS, KAT, U2, random_pattern, strings_near
from program_replay import Dfa2ItemsReplay, Dfa2Replay, DfaReplay, NfaReplay, SampledReplay, host_pipeline_sources
from pyoracle import OracleError, OracleRegex


def _same_table(o, r, sample=None):
    assert (o.states_n, o.initial, o.set_class) == (r.states_n, r.initial, r.set_class)
    assert o.finals() == r.finals()
    states = range(o.states_n) if sample is None else sample
    for s in states:
        for c in range(128):
            assert o.row(s, c) == r.row(s, c), (s, c)


def test_front_end_builds_the_reference_table_kat():
    for k in KAT["kat"]:
        _same_table(OracleRegex(k["pattern"]), rr.RRegex(k["pattern"]))


def test_front_end_builds_the_reference_table_big():
    rng = random.Random(5)
    for k in KAT["big_states"]:
        o = OracleRegex(k["pattern"])
        r = rr.RRegex(k["pattern"])
        assert r.states_n == k["states_n"] and r.set_class == 0
        _same_table(o, r, sample=[0, 1, 2, o.states_n - 1] + [rng.randrange(o.states_n) for _ in range(40)])


def test_front_end_random_patterns_match_oracle_tables():
    rng = random.Random(11)
    n_ok = 0
    for _ in range(300):
        p = random_pattern(rng)
        try:
            o = OracleRegex(p)
        except OracleError:
            with pytest.raises(rr.RRegexError):
                rr.RRegex(p)
            continue
        if o.states_n > 400:
            continue
        try:
            r = rr.RRegex(p)
        except rr.RRegexError as e:
            assert "too large" in str(e), (p, e)
            continue
        _same_table(o, r)
        n_ok += 1
    assert n_ok > 150


@pytest.mark.parametrize("p", ["a)", "|a", "a|", "()", "*a", "?", "+", "a{2", "[", "a{", "caf\xe9", "(|a)", "a(|b)"])
def test_errors_match_oracle(p):
    with pytest.raises(OracleError):
        OracleRegex(p)
    with pytest.raises(rr.RRegexError):
        rr.RRegex(p)


def test_error_messages_of_the_reference_are_kept():
    # Parser.cpp:36 and Parser.cpp:155
    with pytest.raises(rr.RRegexError, match="invalid expression!"):
        rr.RRegex("[")
    with pytest.raises(rr.RRegexError, match="invalid expression"):
        rr.RRegex("a)")


def _replays(r):
    out = []
    for kind, cls in ((rr.ENGINE_NFA, NfaReplay), (rr.ENGINE_DFA, DfaReplay)):
        w = r.program(kind)
        if w is not None:
            out.append(cls(w))
    assert out
    return out


def test_programs_keep_the_language_kat():
    for k in KAT["kat"]:
        r = rr.RRegex(k["pattern"])
        for rep in _replays(r):
            for t in k["accepts"]:
                assert rep.accepts(t.encode("latin-1")), (k["pattern"], t, type(rep).__name__)
            for t in k["rejects"]:
                assert not rep.accepts(t.encode("latin-1")), (k["pattern"], t, type(rep).__name__)


def test_programs_keep_the_language_random():
    rng = random.Random(23)
    checked = 0
    for _ in range(250):
        p = random_pattern(rng)
        try:
            o = OracleRegex(p)
        except OracleError:
            continue
        if o.states_n > 300:
            continue
        try:
            r = rr.RRegex(p)
        except rr.RRegexError:
            continue
        reps = _replays(r)
        for t in strings_near(rng, o):
            want = o.accepts(t)
            for rep in reps:
                assert rep.accepts(t.encode()) == want, (p, t, type(rep).__name__)
            checked += 1
    assert checked > 5000


def test_block_program_beyond_4096_positions():
    """(a|b)*a(a|b){5000}: 5003 positions, no table form -> the group engine (r4: up to 8192 positions, 32 lanes x 5 words); forced
    onto the wave-resident engine here, which AUTO takes beyond that (the reference's Roaring class at any size, Parser.cpp:165).  Its program (exception edges as CSR lists) replays to the oracle's
    answers, in the plain and in the line-mode form; small automata forced onto the engine do too."""
    import numpy as np
    rng = random.Random(43)
    p = "(a|b)*a(a|b){5000}"
    assert rr.RRegex(p).engine_name == "nfa-group-cooperative" and rr.RRegex("(a|b)*a(a|b){8200}").engine_name == "nfa-wave-resident"
    r = rr.RRegex(p, rr.ENGINE_NFA_BLOCK)
    assert r.engine == rr.ENGINE_NFA_BLOCK and r.engine_name == "nfa-wave-resident"
    w = r.program(rr.ENGINE_NFA_BLOCK)
    assert w[1] > 4096
    rep = NfaReplay(w, sparse=True)
    o = OracleRegex(p)
    texts = ["", "a", "a" + "b" * 5000, "b" + "b" * 5000, "ab" * 100 + "a" + "a" * 5000, "a" * 4999, "a" * 5002]
    texts.append("".join(rng.choice("ab") for _ in range(5600)))
    for t in texts:
        assert rep.accepts(t.encode()) == o.accepts(t), len(t)
    data = ("\n".join(texts[:5])).encode()
    assert rep.match_lines(data) == list(o.match_lines(np.frombuffer(data, dtype=np.uint8)))
    for q in ("(ab|cd)+e?", "a{2,9}b", "[ab]*c[ab]{3}"):
        rep = NfaReplay(rr.RRegex(q, rr.ENGINE_NFA_BLOCK).program(rr.ENGINE_NFA_BLOCK), sparse=True)
        oq = OracleRegex(q)
        for t in strings_near(rng, oq, alphabet="abcde"):
            assert rep.accepts(t.encode()) == oq.accepts(t), (q, t)


def test_profiled_order_of_the_stride2_table():
    """order_dfa2 (table_order.cpp) through its host-side entry: on a sample of URL text - 256 lanes, 32 consecutive ones 4 KiB apart
    as a half-wave's stripes are - the search must return two permutations (state 0 stays in slot 0), must not raise the
    conflict figure it minimises, and must lower it on this text; the logical program (and so every replay) is untouched.
    A second call, or a call after the order was decided, is refused."""
    import numpy as np
    import synth
    text = synth.corpus("url", 2, 8 * 32 * 4096)
    stripes = text.reshape(-1, 4096)
    sample = np.ascontiguousarray(stripes[:256, :256])
    r = rr.RRegex(U2)
    before_words = r.program(rr.ENGINE_DFA2).copy()
    assert r.table_order is None and r.program(rr.PROGRAM_DFA2_ORDER) is None
    b, a = r.order_table(sample, 256, 256)
    assert 1.5 < a < b < 4.0, (b, a)
    assert b - a > 0.1                                   # URL text: 2.9 -> 2.5-2.6 distinct entries in the fullest bank
    w = r.program(rr.PROGRAM_DFA2_ORDER)
    D, Cn = int(w[0]), int(w[1])
    rows, cols = w[2:2 + D], w[2 + D:2 + D + Cn]
    assert sorted(rows) == list(range(D)) and sorted(cols) == list(range(Cn)) and rows[0] == 0
    assert (rows != np.arange(D)).any() or (cols != np.arange(Cn)).any()
    assert (r.program(rr.ENGINE_DFA2) == before_words).all()
    with pytest.raises(rr.RRegexError, match="decided"):
        r.order_table(sample, 256, 256)
    # a table small enough to be replicated keeps its order (interleaved copies already keep lanes apart)
    small = rr.RRegex(EMAIL)
    assert small.order_table(sample, 256, 256) is None


def test_arepeat_on_the_cooperative_programs():
    """a{1,300} forced onto the group and block engines (the command of round 2 whose GPU run went silent: VERDICT r2 weak
    #3): both programs are the 301-position chain without exception edges, and their line-mode replay over a sample of the
    synthetic `arepeat` corpus gives the oracle's vector - the host side of that run is sound."""
    import numpy as np
    import synth
    data = synth.corpus("arepeat", 3, 48 << 10)
    want = list(OracleRegex("a{1,300}").match_lines(data))
    for e, sparse in ((rr.ENGINE_NFA_WAVE, False), (rr.ENGINE_NFA_BLOCK, True)):
        r = rr.RRegex("a{1,300}", e)
        w = r.program(e)
        assert (int(w[0]), int(w[1]), int(w[2])) == (10, 301, 0)
        assert NfaReplay(w, sparse=sparse).match_lines(data.tobytes()) == want


def test_line_mode_nfa_step_random():
    """The batch kernel's NFA step as LineNfaEngine runs it (no CHAIN mask thanks to the gap positions, a 1 injected into
    position 0 on every byte, B['\\n'] = {position 0}) replayed over whole corpora against the oracle."""
    import numpy as np
    rng = random.Random(29)
    checked = 0
    for _ in range(200):
        p = random_pattern(rng)
        try:
            o = OracleRegex(p)
        except OracleError:
            continue
        if o.states_n > 300:
            continue
        try:
            r = rr.RRegex(p, rr.ENGINE_NFA)
        except rr.RRegexError:
            continue
        rep = NfaReplay(r.program(rr.ENGINE_NFA))
        lines = strings_near(rng, o) + ["", ""]
        data = ("\n".join(lines) + ("\n" if rng.random() < 0.5 else "")).encode()
        want = list(o.match_lines(np.frombuffer(data, dtype=np.uint8)))
        assert rep.match_lines(data) == want, p
        checked += len(want)
    assert checked > 5000
    for p in (U2, EMAIL, K1000_CONTAINS, "a{1,300}", "(a|b)*a(a|b){40}"):
        o = OracleRegex(p)
        rep = NfaReplay(rr.RRegex(p, rr.ENGINE_NFA).program(rr.ENGINE_NFA))
        lines = ["http://example.com", "a@b", "a" * 300, "a" * 301, "x k17 y", "ab" * 30, "a" + "b" * 40, "", "https://a.b.cd:80/x?y#z"]
        data = ("\n".join(lines)).encode()
        assert rep.match_lines(data) == list(o.match_lines(np.frombuffer(data, dtype=np.uint8))), p[:20]


def test_programs_keep_the_language_configs():
    rng = random.Random(3)
    cases = {
        EMAIL: ["john.doe_1@mail.example.com", "john@", "@x", "a@b c", "a@b", "a.b@c.d.e", "@", "a@@b", ""],
        U2: ["https://www.example.com:8080/a/b/c.html?x=1&y=2#frag", "http://example.com", "http://example",
             "gopher://example.com/", "ftp://a.bc", "ftp://a.b", "http://a-b.c-d.ef:1/x//y?#", "https://a.b.c.d.ef",
             "http://abcdefghijklmnopq.com", "http://abcdefghijklmnop.com", "http://x.com:123456", ""],
        "a{1,300}": ["", "a", "a" * 299, "a" * 300, "a" * 301, "a" * 400, "a" * 150 + "b"],
        K1000: ["k1", "k1000", "k1001", "k0", "k999", "k", "k01", "k100", "kk1", "k10 ", ""],
        K1000_CONTAINS: ["GET /index k17 200", "xk1", "k", "no keyword here", "k0 k", "zzk1000zz", ""],
    }
    for p, texts in cases.items():
        o = OracleRegex(p)
        r = rr.RRegex(p)
        for rep in _replays(r):
            for t in texts:
                assert rep.accepts(t.encode()) == o.accepts(t), (p[:30], t, type(rep).__name__)


def test_reduction_statistics():
    # what the compaction buys on the BASELINE configs (documented in DESIGN.md)
    r = rr.RRegex(U2)
    assert r.states_n == 226 and r.useful_states == 83 and r.byte_classes == 16
    assert r.words_per_set == 3
    r = rr.RRegex("a{1,85}", rr.ENGINE_NFA)
    w = r.program(rr.ENGINE_NFA)
    assert w[1] == 86 and w[2] == 0           # a pure shift chain: no exception rows
    r = rr.RRegex(K1000)
    assert r.states_n == 7786 and r.engine == rr.ENGINE_DFA and r.engine_name == "dfa-stride2-table"


def test_wave_program_for_automata_beyond_one_lane():
    """> 512 positions and an exploding subset construction: AUTO falls through to the wave-cooperative NFA
    (the Roaring class).  Its program (no carry groups) replays to the oracle's answers."""
    rng = random.Random(41)
    for p, alphabet, lens in [("(a|b)*a(a|b){600}", "ab", (598, 601, 602, 640)), ("a{1,900}", "a", (1, 899, 900, 901, 950)),
                              ("(ab|cd){2,300}e", "abcde", (5, 401, 601, 603))]:
        o = OracleRegex(p)
        r = rr.RRegex(p)
        if p.startswith("(a|b)"):
            assert r.engine == rr.ENGINE_NFA_WAVE and r.engine_name == "nfa-group-cooperative"
        w = rr.RRegex(p, rr.ENGINE_NFA_WAVE).program(rr.ENGINE_NFA_WAVE)
        assert w is not None and w[1] > 512
        rep = NfaReplay(w)
        texts = ["", alphabet[0]]
        for n in lens:
            texts.append("".join(rng.choice(alphabet) for _ in range(n)))
            texts.append(alphabet[0] * n)
            texts.append(("ab" * n)[:n] if "b" in alphabet else alphabet[0] * n)
        if p.startswith("(ab|cd)"):
            texts += ["ab" * 150 + "e", "abcd" * 150 + "e", "ab" * 301 + "e", "ab" + "e", "abab" + "e"]
        for t in texts:
            assert rep.accepts(t.encode()) == o.accepts(t), (p, len(t))


def test_stride2_program_keeps_the_language():
    """The two-bytes-per-step table (pair columns + T2) against the oracle, line by line, incl. line ends on either
    byte of a pair, empty lines, odd and even corpus lengths."""
    import numpy as np
    rng = random.Random(51)
    pats = [EMAIL, U2, "a{1,300}", K1000, "abc", "a*", "(ab|cd)+e?", "[ab]+c[ab]*"]
    for _ in range(25):
        p = random_pattern(rng)
        try:
            OracleRegex(p)
            if rr.RRegex(p).program(rr.ENGINE_DFA2) is not None:
                pats.append(p)
        except (OracleError, rr.RRegexError):
            pass
    for p in pats:
        o = OracleRegex(p)
        w = rr.RRegex(p).program(rr.ENGINE_DFA2)
        assert w is not None, p
        rep = Dfa2Replay(w)
        for trial in range(6):
            lines = [random_pattern_text(rng, p) for _ in range(rng.randint(0, 12))]
            data = "\n".join(lines).encode()
            if trial % 2:
                data += b"\n"
            if trial == 4:
                data = b"\n\n" + data + b"\n\n\n"
            want = list(o.match_lines(np.frombuffer(data, dtype=np.uint8))) if data else []
            assert rep.match_lines(data) == want, (p[:30], data[:60])


def test_stride2_items_program_keeps_the_language():
    """The stride-2 table of explicit items with separators (rrx_program_words kind 15: '\\n' an ordinary byte, code 128 the end of
    an item) against the oracle's whole-string acceptance, item by item: items that hold '\\n', 0x00 and bytes >= 0x80, empty items,
    ends on either code of a pair."""
    rng = random.Random(52)
    pats = [EMAIL, U2, "a{1,300}", K1000, "abc", "a*", ".*", "a.c", "[^a]+", "(ab|cd)+e?", "[ab]+c[ab]*"]
    for _ in range(25):
        p = random_pattern(rng)
        try:
            OracleRegex(p)
            if rr.RRegex(p).program(rr.PROGRAM_DFA2_ITEMS) is not None:
                pats.append(p)
        except (OracleError, rr.RRegexError):
            pass
    for p in pats:
        o = OracleRegex(p)
        w = rr.RRegex(p).program(rr.PROGRAM_DFA2_ITEMS)
        assert w is not None, p
        rep = Dfa2ItemsReplay(w)
        for trial in range(6):
            items = []
            for _ in range(rng.randint(0, 12)):
                b = bytearray(random_pattern_text(rng, p).encode())
                if b and rng.random() < 0.3:
                    b[rng.randrange(len(b))] = rng.choice([10, 10, 0, 0x80, 0xff, 0x7f])
                items.append(bytes(b))
            want = [1 if (not any(c == 0 or c >= 0x80 for c in it) and o.accepts(it)) else 0 for it in items]
            assert rep.match_items(items) == want, (p[:30], items[:6])
    assert rr.RRegex("abc", rr.ENGINE_DFA).program(rr.PROGRAM_DFA2_ITEMS) is None       # (the byte-stride engine has no stride-2 table)


def random_pattern_text(rng, p):
    alphabet = "abcxk01.d@:/e" if len(p) < 60 else "abcdefghijklmnopqrstuvwxyz0123456789.:/-?#=&_~%@ "
    return "".join(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 2, 3, 5, 8, 13, 30])))


def test_host_pipeline_is_clean_under_asan_and_ubsan(tmp_path):
    """Sanitizers run on the CPU build only: the host compile pipeline (front end + every lowering + the packing of every
    device image) is plain C++, so it is built here with g++ -fsanitize=address,undefined and driven with the known answers,
    the big configs, broken patterns and random patterns.  Any report aborts the driver (-fno-sanitize-recover), and so does
    a packed image that does not decode back to its program."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "roaringregex_amd", "csrc")
    exe = str(tmp_path / "host_pipeline_asan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I", csrc,
                           os.path.join(root, "tests", "cpp", "host_pipeline_driver.cpp")] + host_pipeline_sources() + ["-o", exe])
    rng = random.Random(2024)
    pats = [k["pattern"] for k in KAT["kat"]] + [b["pattern"] for b in KAT["big_states"]]
    pats += [EMAIL, U2, "a{1,300}", "(a|b)*a(a|b){12}", "(a|b)*a(a|b){40}", K1000_CONTAINS]
    from table_edge_cases import CASES                    # the automata on a table form's limit, and the first ones beyond it
    pats += sorted({c.pattern for c in CASES if c.side in ("at", "past")})
    pats += ["(", ")", "a)", "(a", "[", "[a", "a{", "a{2", "a{2,", "a{,}", "a{3,2}", "*", "+a", "a||b", "\\", "a\\", "[]", "[^]", "a{0}", "a{0,0}", "()", "(|)", ""]
    pats += [random_pattern(rng) for _ in range(150)]
    pats = [p for p in pats if "\n" not in p]
    out = subprocess.run([exe], input=("\n".join(pats) + "\n").encode("latin-1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode("latin-1")[-3000:]
    lines = out.stdout.decode("latin-1").splitlines()
    assert lines[-1].startswith("done %d " % len(pats)), lines[-1]
    # every device image form was packed, bound to a host copy and decoded back against its program at least once
    packed = lines[-2].split()
    assert packed[0] == "packed" and all(int(v) >= 1 for v in packed[2::2]), lines[-2]
    # the sanitized build must agree with the shipped library on what compiles, and on the engine and table form AUTO chooses
    for p, line in zip(pats, lines):
        engine_name = "none"
        try:
            engine_name = rr.RRegex(p).engine_name
            ok = True
        except rr.RRegexError as e:
            ok = "too large" in str(e)               # compiled, but no device engine admits it
        assert ok == (" ok " in line), (p[:60], line)
        if ok:
            assert line.rsplit(" engine ", 1)[1] == engine_name, (p[:60], line, engine_name)


def test_table_forms_are_the_recorded_ones():
    """Which engine a pattern gets and which forms its match table and its contains table take (csrc/plan.cpp) are pinned, for
    the known-answer patterns and the fixed patterns under AUTO and every table engine, to tests/golden/table_forms.json
    (make_table_forms.py): a change of a fit rule or of AUTO's order shows here, without a GPU."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_forms.json")) as f:
        golden = json.load(f)
    recorded = {e["pattern"] for e in golden["forms"]}
    for p in [k["pattern"] for k in KAT["kat"]] + [b["pattern"] for b in KAT["big_states"]] + [EMAIL, U2, K1000, K1000_CONTAINS]:
        assert p in recorded, p[:60]
    assert {"ENGINE_AUTO", "ENGINE_DFA", "ENGINE_DFA_GLOBAL", "ENGINE_DFA2"} <= set(golden["engines"])
    names = set()
    for entry in golden["forms"]:
        p = entry["pattern"]
        for engine, want in zip(golden["engines"], entry["by_engine"]):
            try:
                r = rr.RRegex(p, getattr(rr, engine))
            except rr.RRegexError:
                assert want is None, (p[:60], engine, want)
                continue
            try:
                contains = r.contains_engine_name
            except rr.RRegexError:
                contains = None
            assert [r.engine, r.engine_name, contains, r.contains_states] == want, (p[:60], engine, want)
            names.update((("match", r.engine_name), ("contains", contains)))
    # the fixture reaches every form of both tables
    for form in ("dfa-stride2-table", "dfa-wide-table", "dfa-classed-table", "dfa-global-table"):
        assert ("match", form) in names and ("contains", form) in names, form


def test_search_tables_find_the_earliest_ending_leftmost_match():
    """Search has no counterpart in the reference's code; it is pinned to the reference's ACCEPTANCE:
    the oracle tries every substring with whole-string acceptance (smallest end, then smallest start).  The forward
    and reverse tables are replayed on the CPU exactly as the device kernel runs them."""
    from program_replay import SearchLineReplay, SearchLine2Replay, SearchReplay
    rng = random.Random(31)
    pats = ["ab+c", "a*", "(a|b)*abb", "[0-9]+\\.[0-9]+", "x?y?z?", "k(1|10|100)", "a{2,4}b", ".*c", "c.*", "(ab|b)a?", "[^a]b", EMAIL, U2]
    done = 0
    while done < 40:
        p = random_pattern(rng)
        try:
            if OracleRegex(p).states_n <= 120:
                pats.append(p)
                done += 1
        except OracleError:
            pass
    for p in pats:
        o = OracleRegex(p)
        r = rr.RRegex(p)
        fw, rv = r.program(rr.PROGRAM_SEARCH_FWD), r.program(rr.PROGRAM_SEARCH_REV)
        assert fw is not None and rv is not None, p
        rep = SearchReplay(fw, rv)
        # what the walk-back of search_chunks_kernel relies on (it steps on to the end of its four-byte turn after dying): state 0
        # of the reverse table is dead for good and not accepting, and a doubled class still fits a byte
        assert not rep.r.acc[0] and not rep.r.next[0].any() and rep.r.ncls <= 128, p
        alphabet = "abcxk01.d@yz" if p not in (EMAIL, U2) else "ab1.@:/hftps"
        lines = [bytes(ord(ch) for ch in "".join(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 2, 5, 9, 14])))) for _ in range(60)]
        if p == U2:
            lines += [b"see http://a.b/c ok", b"xxftp://h.io", b"https://"]
        lines += [b"\x80ab" + lines[0], lines[1] + b"\xc3\xa9" + lines[2]]          # bytes outside the domain are ordinary text
        st, en = o.search_lines(b"\n".join(lines) + b"\n")
        lw = r.program(rr.PROGRAM_SEARCH_LINE)               # the stripe-wise kernel's table (absent for patterns that accept "")
        line_rep = SearchLineReplay(lw, rv) if lw is not None else None
        assert (line_rep is None) == o.accepts(""), p
        l2 = r.program(rr.PROGRAM_SEARCH_LINE2)              # ... and its stride-2 form, what the kernel steps
        line2_rep = SearchLine2Replay(l2, rv) if l2 is not None else None
        assert (line2_rep is None) == (line_rep is None), p
        if line2_rep is not None:
            assert line2_rep.layout == 1, (p, "these tables fit the LDS")
        for ln, s, e in zip(lines, st, en):
            assert rep.search(ln) == (int(s), int(e)), (p[:50], ln, (int(s), int(e)))
            if line_rep is not None:
                assert line_rep.search(ln) == (int(s), int(e)), (p[:50], ln, (int(s), int(e)), "line form")
                for lead in (0, 1):
                    assert line2_rep.search(ln, lead) == (int(s), int(e)), (p[:50], ln, (int(s), int(e)), "stride-2 line form", lead)
        cnt, ast, aen = o.search_all(b"\n".join(lines) + b"\n")
        k = 0
        for ln, c in zip(lines, cnt):
            want = [(int(ast[k + j]), int(aen[k + j])) for j in range(int(c))]
            assert rep.search_all(ln) == want, (p[:50], ln, want)
            if line2_rep is not None:
                for lead in (0, 1):
                    assert line2_rep.search_all(ln, lead) == want, (p[:50], ln, want, "stride-2 line form", lead)
            k += int(c)
        # the forward table alone (RRX_OPT_SEARCH_ANCHORED 0; what a product beyond the row budget falls back to): no hit is anchored
        if line2_rep is not None:
            r0 = rr.RRegex(p)
            r0.set_search_anchored(False)
            l0 = SearchLine2Replay(r0.program(rr.PROGRAM_SEARCH_LINE2), rv)
            assert l0.nrows <= line2_rep.nrows and not ((l0.first >> 24) & 0b0101 & ((l0.first >> 25) & 0b0101)).any(), p
            for ln, s, e in zip(lines, st, en):
                assert l0.search(ln, 1) == (int(s), int(e)), (p[:50], ln, "forward table alone")
            try:
                r.set_search_anchored(False)
                raise AssertionError("the option must be refused once the tables are built")
            except rr.RRegexError:
                pass


# ---------------------------------------------------------------------------------------------------------------------------
# Large bounded repeats: the reference builds x{m,n} by plain copies and resolves every eps-edge of the fold
# eagerly (Parser.cpp:123-141, NFA.cc:108-121, 172-185): n^2/2 edges.  The front end keeps rows as shared pieces, trim() drops the
# dominated skip edges from the pieces; both must stay exact.

def nullable_heavy_pattern(rng, depth=0):
    """Random patterns dense in what makes the fold quadratic: optional / starred / {0,n} / {1,n} operands, nested."""
    parts = []
    for _ in range(rng.randint(1, 3 if depth else 4)):
        r = rng.random()
        if depth < 3 and r < 0.45:
            alts = [nullable_heavy_pattern(rng, depth + 1) for _ in range(rng.randint(1, 2))]
            atom = "(" + "|".join(alts) + ")"
        else:
            atom = rng.choice(["a", "b", "c", "[ab]", "[bc]", "."])
        q = rng.random()
        if q < 0.20:
            atom += "?"
        elif q < 0.32:
            atom += "*"
        elif q < 0.40:
            atom += "+"
        elif q < 0.62:
            atom += "{%d,%d}" % (rng.randint(0, 1), rng.randint(2, 7))
        elif q < 0.70:
            atom += "{%d}" % rng.randint(2, 4)
        parts.append(atom)
    return "".join(parts)


def test_nested_nullable_repeats_build_the_reference_table():
    rng = random.Random(77)
    n_ok = 0
    for _ in range(400):
        p = nullable_heavy_pattern(rng)
        try:
            o = OracleRegex(p)
        except OracleError:
            continue
        if o.states_n > 700:
            continue
        r = rr.RRegex(p)
        _same_table(o, r, sample=None if o.states_n <= 250 else [0, 1, o.states_n - 1] + [rng.randrange(o.states_n) for _ in range(60)])
        for rep in _replays(r):
            for t in strings_near(rng, o, alphabet="abc", tries=30, maxlen=16):
                assert rep.accepts(t.encode()) == o.accepts(t), (p, t, type(rep).__name__)
        n_ok += 1
    assert n_ok > 250


@pytest.mark.parametrize("p,alphabet", [
    ("(ab){1,40}", "ab"), ("(abc|de){1,25}", "abcde"), ("(a+b+){1,12}", "ab"), ("(a{0,3}b{0,3}){1,9}", "ab"),
    ("([ab]{1,10}c?){1,8}", "abc"), ("(a{1,9}){1,9}", "a"), ("(abcdefghij){1,9}", "abcdefghij"), ("((ab){1,5}c){1,6}x?", "abcx"),
    ("(a?b?c?){1,12}", "abc"), ("((a|b)*a(a|b){3}){1,10}", "ab"), ("(k1|k2|k10|k11|k12){1,6}", "k012"), ("(a*b*){1,7}x", "abx"),
    ("(a?|b?c)*{1,9}", "abc"), ("((a|b)?(c|d)?){1,11}x", "abcdx"), ("(.?a){1,9}", "ab"), ("(a|bc?)+{1,6}", "abc")])
def test_repeat_families_keep_the_language(p, alphabet):
    """The families the domination proofs of trim() are made for, at sizes the oracle finishes: every device program accepts
    exactly what the oracle accepts, on random strings, mutations of accepted ones and long runs."""
    rng = random.Random(len(p) * 7919)
    o = OracleRegex(p)
    r = rr.RRegex(p)
    reps = _replays(r)
    for e in (rr.ENGINE_NFA_WAVE, rr.ENGINE_NFA_BLOCK):
        reps.append(NfaReplay(rr.RRegex(p, e).program(e), sparse=(e == rr.ENGINE_NFA_BLOCK)))
    texts = strings_near(rng, o, alphabet=alphabet, tries=120, maxlen=30)
    texts += ["".join(rng.choice(alphabet) for _ in range(rng.randint(20, 120))) for _ in range(40)]
    texts += [(alphabet[:k] * 200)[:n] for k in (1, 2, len(alphabet)) for n in (17, 18, 19, 20, 40, 80, 81, 90, 91, 120)]
    if p.startswith("(k1|"):
        kws = ["k1", "k2", "k10", "k11", "k12"]
        texts += ["".join(rng.choice(kws) for _ in range(n)) for n in (1, 2, 3, 5, 6, 7, 8) for _ in range(4)]
    seen_accept = False
    for t in texts:
        want = o.accepts(t)
        seen_accept = seen_accept or want
        for rep in reps:
            assert rep.accepts(t.encode()) == want, (p, t, type(rep).__name__)
    assert seen_accept


def test_compile_time_of_large_repeats_is_bounded():
    """Every pattern the front end admits compiles in seconds (the round-3 pipeline: a{1,9600} 126 s, (ab){1,2400} 289 s)."""
    import time
    cases = [("a{1,20000}", 20001), ("[ab]{1,20000}", 20001), ("(ab){1,5000}", 10001), ("(abc|de){1,3000}", 12002),
             ("(a+b+){1,5000}", 20001), ("(abcdefghij){1,3000}", 30001), ("(a{0,3}b{0,3}){1,1500}", 12001), ("(a{1,100}){1,100}", 10001),
             ("([ab]{1,40}c?){1,200}", 8201), ("(a?){20000}", 20001), ("((a|b)*a(a|b){10}c?){1,1000}", 13001)]
    for p, useful in cases:
        t0 = time.time()
        r = rr.RRegex(p)
        dt = time.time() - t0
        assert dt < 5.0, (p, dt)
        assert r.useful_states == useful, (p, r.useful_states)
    # closed form: a{1,20000} accepts a^n for 1 <= n <= 20000 and nothing else
    r = rr.RRegex("a{1,20000}")
    assert r.states_n == 59999 and r.engine_name == "nfa-wave-resident"
    rep = NfaReplay(r.program(rr.ENGINE_NFA_BLOCK), sparse=True)
    for n, want in ((0, False), (1, True), (2, True), (19999, True), (20000, True), (20001, False), (20500, False)):
        assert rep.accepts(b"a" * n) == want, n
    assert not rep.accepts(b"a" * 700 + b"b" + b"a" * 700)
    # the expanded rows are the reference's (the n^2/2 edges, on demand): the second copy's initial state reaches the state
    # behind `a` and the initial state of every later copy, the one after it two fewer (a{1,6}: [3,5,6,8,...,15], [6,8,...,15])
    assert r.row(0, ord("a")) == [1, 2] and not r.row(0, ord("b")) and not r.row(1, ord("a"))
    row = r.row(2, ord("a"))
    assert len(row) == 39997 and row[:6] == [3, 5, 6, 8, 9, 11] and row[-1] == 59997
    assert r.row(5, ord("a")) == row[2:]
    # (ab){1,5000} determinises into a chain: exactly the table a hand-written matcher would use
    r = rr.RRegex("(ab){1,5000}")
    rep = DfaReplay(r.program(rr.ENGINE_DFA))
    for n in (0, 1, 2, 4999, 5000, 5001):
        assert rep.accepts(b"ab" * n) == (1 <= n <= 5000), n
    assert not rep.accepts(b"ab" * 10 + b"a")


def test_budget_refusal_is_an_error_not_a_hang():
    """What the pipeline will not build within its work budget is refused with RRX_ERR_UNSUPPORTED in seconds.  A sequence of n
    DIFFERENT optional keywords needs its n^2/2 skip edges (no copy stands in for another): 1500 of them compile, 2600 exceed
    the edge budget (lower.hpp: kTrimBudget)."""
    import ctypes as C
    import time
    L = rr._L
    ok = "".join("(k%d)?" % i for i in range(1, 1501))
    t0 = time.time()
    r = rr.RRegex(ok)
    assert time.time() - t0 < 5.0 and r.states_n == 14286
    rep = DfaReplay(r.program(rr.ENGINE_DFA))
    for t, want in (("", True), ("k1", True), ("k1k2", True), ("k2k1", False), ("k7k900k1500", True), ("k1500k1", False), ("k15", True), ("k1501", False)):
        assert rep.accepts(t.encode()) == want, t
    big = "".join("(k%d)?" % i for i in range(1, 2601))
    h = C.c_void_p()
    t0 = time.time()
    rc = L.rrx_compile(big.encode(), C.byref(h))
    assert rc == 4 and time.time() - t0 < 5.0                      # RRX_ERR_UNSUPPORTED
    assert b"work budget" in L.rrx_last_error()
    with pytest.raises(rr.RRegexError, match="too many states"):   # RRX_ERR_PATTERN: beyond the front end's 65536 states
        rr.RRegex("(a|b)*a(a|b){20000}")


def test_sampled_table_decides_exactly_or_not_at_all():
    """lower_dfa_sampled (README.md:18-21: the live sets met on real text are few): U2(x|y)*x(x|y){30} and
    (U2)|(x|y)*x(x|y){30} do not determinise (2^31 sets on x/y text) and AUTO leaves them on the NFA lane engine; a table over the
    sets a URL text sample reaches has about a hundred states.  Every line it DECIDES has the oracle's verdict, the others end in
    the ESCAPE state; text like the sample is decided throughout, x/y tails escape; the stride-2 form with two result bits per
    line end says the same line by line."""
    import synth
    rng = random.Random(9)
    url = synth.corpus("url", 3, 2 << 20)
    lines = url.tobytes().split(b"\n")[:-1]
    for pattern in (U2 + "(x|y)*x(x|y){30}", "(" + U2 + ")|(x|y)*x(x|y){30}"):
        o = OracleRegex(pattern)
        r = rr.RRegex(pattern)
        assert r.engine == rr.ENGINE_NFA and r.sampled_table is None and r.program(rr.PROGRAM_SAMPLED_DFA) is None
        states, open_tr = r.learn_table(url[:1 << 16])
        assert 20 < states < 2000 and open_tr > 0
        with pytest.raises(rr.RRegexError):
            r.learn_table(url[:1 << 16])                           # decided once
        rep = SampledReplay(r.program(rr.PROGRAM_SAMPLED_DFA), r.program(rr.PROGRAM_SAMPLED_DFA2))
        assert int(rep.esc.sum()) == 1 and not rep.acc[np.nonzero(rep.esc)[0][0]]
        like = lines[2000:6000]                                      # (beyond the 64 KiB the table was learnt from)
        # what escapes: x/y runs the sample never showed - behind a VALID url for the first pattern, on their own for the second
        valid = [ln for ln in lines[6000:9000] if OracleRegex(U2).accepts(ln.decode("latin-1"))][:300]
        tails = [ln + bytes(rng.choice(b"xy") for _ in range(rng.randint(20, 80))) for ln in valid] + \
                [bytes(rng.choice(b"xy") for _ in range(rng.randint(1, 80))) for _ in range(300)] + [b"", b"x" * 31, b"xy" * 40]
        decided = escaped = 0
        for ln in like + tails:
            v = rep.verdict(ln)
            if v is None:
                escaped += 1
            else:
                decided += 1
                assert v == int(o.accepts(ln.decode("latin-1"))), (pattern[-20:], ln)
        assert sum(rep.verdict(ln) is None for ln in like) <= len(like) // 50, "text like the sample hardly escapes (x/y runs in a path do)"
        assert escaped > 50 and decided > 4000
        data = b"\n".join(like[:600] + tails[:80]) + b"\n"
        assert rep.match_lines2(data) == [rep.verdict(ln) for ln in like[:600] + tails[:80]]
    # a table its OWN sample escapes from is not installed (every escaped line is read twice): (a|b)*a(a|b){40} over random a/b lines
    # meets a new set on every line
    ab = np.frombuffer(b"\n".join(bytes(rng.choice(b"ab") for _ in range(rng.randint(60, 120))) for _ in range(600)) + b"\n", dtype=np.uint8)
    r = rr.RRegex("(a|b)*a(a|b){40}")
    assert r.engine == rr.ENGINE_NFA
    with pytest.raises(rr.RRegexError, match="2 %"):
        r.learn_table(ab)
    assert r.sampled_table is None and r.program(rr.PROGRAM_SAMPLED_DFA) is None
    # an automaton that determinises has no use for a sampled table; a forced engine is left alone
    with pytest.raises(rr.RRegexError, match="AUTO"):
        rr.RRegex(U2).learn_table(url[:4096])
    with pytest.raises(rr.RRegexError, match="AUTO"):
        rr.RRegex(U2 + "(x|y)*x(x|y){30}", rr.ENGINE_NFA).learn_table(url[:4096])
