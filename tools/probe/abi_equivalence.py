"""What a pattern compiles to in two builds of librrx.so, record by record, no GPU: the check behind
profiles/abi_split_equivalence.txt (and, without the sampled table, behind the two equivalence files before it).

    python tools/probe/abi_equivalence.py PARENT/roaringregex_amd/librrx.so roaringregex_amd/librrx.so [--random 2000] [--out DIR]

Each library is loaded in a child process of its own.  Patterns: tests/golden/kat.json (kat and big_states), the fixed patterns of
tests/patterns.py, the bench.py workload patterns, the patterns tests/test_abi_errors.py names, a dozen broken and nullable ones,
and --random draws of patterns.random_pattern from random.Random(2024); each under the eight requested engines.  Per compile: return
code and error text, rrx_engine, rrx_engine_name, rrx_contains_engine_name, rrx_contains_states, rrx_accepts_empty, length and
SHA-256 of rrx_program_words for the kinds 0..18.  On every sampled-eligible compile (rrx_learn_table does not answer "serves
automata that AUTO leaves on the NFA lane engine"): rrx_learn_table on one fixed text per pattern - URL text for a pattern that
names a scheme, else seeded lines over the pattern's own letters -, its return code and error text, rrx_sampled_table's three
outputs, a second rrx_learn_table's refusal, and the kinds 12 and 13 again.

After the plain records, in the same file: capture groups - every pattern of the set with a parenthesis, groups 1 up to the number
of '(' in it (3 at most): return code and error text of rrx_group_compile_ex, length and SHA-256 of the three rrx_group_part texts
and of rrx_group_program_words for the kinds 21..24 - and pattern sets - those of tests/multi_cases.py and --sets seeded draws of
1, 2, 5, 16 and 32 members from the pattern list, each under the default and the global form and with max_rows = 64 (several
groups): return code and error text of rrx_multi_compile_ex, rrx_multi_groups, per group its mask, its states and the length and
SHA-256 of rrx_multi_program_words.  (tests/multi_cases.py imports the package: the tree must be built.)"""
import argparse
import collections
import ctypes as C
import hashlib
import json
import os
import random
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ENGINES = {"AUTO": 0, "NFA": 1, "DFA": 2, "DFA_GLOBAL": 3, "NFA_WAVE": 4, "DFA2": 5, "NFA_BLOCK": 8, "NFA_SPARSE": 10}
KINDS = range(19)
GROUP_KINDS = range(21, 25)
SET_FORMS = {"default": (0, 0), "global": (3, 0), "rows64": (0, 64)}       # name -> (engine, max_rows)
SET_SIZES = (1, 2, 5, 16, 32)


def pattern_set(nrandom):
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT]
    import patterns as P
    import bench
    pats = [k["pattern"] for k in P.KAT["kat"]] + [k["pattern"] for k in P.KAT["big_states"]]
    pats += [P.EMAIL, P.U2, P.K1000, P.K1000_CONTAINS] + list(bench.patterns().values())
    text = open(os.path.join(ROOT, "tests", "test_abi_errors.py")).read()
    pats += [m.group(2) for m in re.finditer(r"""(b?)"((?:[^"\\]|\\.)*)\"""", text) if any(ch in m.group(2) for ch in "()[]*+{")][:40]
    pats += ["(", "a)", "[a", "a{2", "a{3,2}", "*a", "a**", "\\", "", "a*", "a?", "(a|b)*", "x?y?z?", "(ab)*", "[0-9]*", "(a*)*", "a{0,3}", "()"]
    rng = random.Random(2024)
    pats += [P.random_pattern(rng) for _ in range(nrandom)]
    return list(collections.OrderedDict.fromkeys(pats))


def pattern_sets(pats, nsets):
    import multi_cases
    sets = [list(v) for v in multi_cases.SETS.values()]
    rng = random.Random(2024)
    return sets + [[rng.choice(pats) for _ in range(SET_SIZES[i % len(SET_SIZES)])] for i in range(nsets)]


def why(rec):
    """A refusal's error text without the pattern or group number it names, cut short: the key the summary counts refusals by."""
    return re.sub(r"^(pattern|group) \d+:? ", r"\1 N ", rec["error"])[:48]


def learn_text(pattern):
    if "http" in pattern:
        sys.path[:0] = [os.path.join(ROOT, "tools")]
        import synth
        return synth.corpus("url", 3, 1 << 16).tobytes()
    letters = sorted(set(ch for ch in pattern if ch.isalpha())) or sorted(set(ch for ch in pattern if ch.isalnum())) or ["a"]
    rng = random.Random(int(hashlib.sha256(pattern.encode()).hexdigest()[:8], 16))
    return b"\n".join("".join(rng.choice(letters) for _ in range(rng.randint(20, 120))).encode() for _ in range(600)) + b"\n"


def child(lib_path, pattern_file, out_path):
    L = C.CDLL(lib_path)
    L.rrx_last_error.restype = C.c_char_p
    L.rrx_engine_name.restype = C.c_char_p
    L.rrx_contains_engine_name.restype = C.c_char_p
    L.rrx_program_words.restype = C.c_size_t
    L.rrx_program_words.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.rrx_learn_table.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.rrx_sampled_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    for f in ("rrx_engine", "rrx_contains_states", "rrx_accepts_empty", "rrx_free"):
        getattr(L, f).argtypes = [C.c_void_p]
    L.rrx_engine_name.argtypes = L.rrx_contains_engine_name.argtypes = [C.c_void_p]

    L.rrx_group_compile_ex.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    L.rrx_group_part.restype = L.rrx_group_program_words.restype = C.c_size_t
    L.rrx_group_part.argtypes = L.rrx_group_program_words.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.rrx_multi_compile_ex.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_void_p]
    L.rrx_multi_groups.restype = L.rrx_multi_program_words.restype = C.c_size_t
    L.rrx_multi_group_mask.restype = L.rrx_multi_group_states.restype = C.c_uint32
    L.rrx_multi_program_words.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.rrx_multi_group_mask.argtypes = L.rrx_multi_group_states.argtypes = [C.c_void_p, C.c_size_t]
    L.rrx_multi_groups.argtypes = L.rrx_group_free.argtypes = L.rrx_multi_free.argtypes = [C.c_void_p]

    def sized(fn, h, which, ctype=C.c_uint32):             # [length, SHA-256] of what a "cap = 0 sizes it" entry returns
        n = fn(h, which, None, 0)
        buf = (ctype * max(n, 1))()
        fn(h, which, buf, n)
        return [n, hashlib.sha256(bytes(buf)[:C.sizeof(ctype) * n]).hexdigest()]

    def words(h, kind):
        return sized(L.rrx_program_words, h, kind)

    work = json.load(open(pattern_file))
    pats = work["patterns"]
    with open(out_path, "w") as out:
        for p in pats:
            for name, eng in ENGINES.items():
                h = C.c_void_p()
                rc = L.rrx_compile_ex(p.encode("latin-1", "replace"), eng, C.byref(h))
                rec = {"pattern": p, "engine": name, "rc": rc}
                if rc:
                    rec["error"] = L.rrx_last_error().decode()
                else:
                    rec.update(engine_no=L.rrx_engine(h), engine_name=L.rrx_engine_name(h).decode(),
                               contains=(L.rrx_contains_engine_name(h) or b"").decode(), contains_states=L.rrx_contains_states(h),
                               accepts_empty=L.rrx_accepts_empty(h), words=[words(h, k) for k in KINDS])
                    text = b"ab\nab\n"
                    rc1 = L.rrx_learn_table(h, text, len(text))
                    if not (rc1 and b"AUTO leaves" in L.rrx_last_error()):          # sampled-eligible: one fresh handle, the pattern's text
                        L.rrx_free(h)
                        h = C.c_void_p()
                        L.rrx_compile_ex(p.encode("latin-1", "replace"), eng, C.byref(h))
                        text = learn_text(p)
                        states, open_tr = C.c_uint32(0), C.c_uint32(0)
                        rc1 = L.rrx_learn_table(h, text, len(text))
                        err1 = L.rrx_last_error().decode() if rc1 else ""
                        st = L.rrx_sampled_table(h, C.byref(states), C.byref(open_tr))
                        rc2 = L.rrx_learn_table(h, text, len(text))
                        rec["sampled"] = {"rc": rc1, "error": err1, "status": st, "states": states.value, "open": open_tr.value,
                                          "again": [rc2, L.rrx_last_error().decode()], "words": [words(h, 12), words(h, 13)]}
                    L.rrx_free(h)
                out.write(json.dumps(rec, sort_keys=True) + "\n")
        for p in pats:
            for group in range(1, min(p.count("("), 3) + 1):
                h = C.c_void_p()
                rc = L.rrx_group_compile_ex(p.encode("latin-1", "replace"), group, 0, C.byref(h))
                rec = {"group_of": p, "group": group, "rc": rc}
                if rc:
                    rec["error"] = L.rrx_last_error().decode()
                else:
                    rec.update(parts=[sized(L.rrx_group_part, h, w, C.c_char) for w in range(3)],
                               words=[sized(L.rrx_group_program_words, h, k) for k in GROUP_KINDS])
                    L.rrx_group_free(h)
                out.write(json.dumps(rec, sort_keys=True) + "\n")
        for n, members in enumerate(work["sets"]):
            arr = (C.c_char_p * len(members))(*[m.encode("latin-1", "replace") for m in members])
            for form, (eng, max_rows) in SET_FORMS.items():
                h = C.c_void_p()
                rc = L.rrx_multi_compile_ex(C.cast(arr, C.c_void_p), len(members), eng, max_rows, C.byref(h))
                rec = {"set": n, "members": len(members), "form": form, "rc": rc}
                if rc:
                    rec["error"] = L.rrx_last_error().decode()
                else:
                    rec["groups"] = [[L.rrx_multi_group_mask(h, g), L.rrx_multi_group_states(h, g)] + sized(L.rrx_multi_program_words, h, g)
                                     for g in range(L.rrx_multi_groups(h))]
                    L.rrx_multi_free(h)
                out.write(json.dumps(rec, sort_keys=True) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=2)
    ap.add_argument("--random", type=int, default=2000)
    ap.add_argument("--sets", type=int, default=250)
    ap.add_argument("--out", default=os.environ.get("PROBE_OUT", os.path.join(ROOT, "probe_out")))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    pats = pattern_set(a.random)
    pfile = os.path.join(a.out, "equivalence_patterns.json")
    sets = pattern_sets(pats, a.sets)
    json.dump({"patterns": pats, "sets": sets}, open(pfile, "w"))
    outs = [os.path.join(a.out, "equivalence_%s.jsonl" % side) for side in ("parent", "tree")]
    kids = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--as-child", lib, pfile, o]) for lib, o in zip(a.libs, outs)]
    assert all(k.wait() == 0 for k in kids), "a child failed"
    A, B = (open(o).read().splitlines() for o in outs)
    differ = sum(x != y for x, y in zip(A, B)) + abs(len(A) - len(B))
    every = [json.loads(x) for x in B]
    recs = [r for r in every if "pattern" in r]
    ok = [r for r in recs if r["rc"] == 0]
    print("patterns %d x engines %d = compiles %d" % (len(pats), len(ENGINES), len(recs)))
    print("compiled %d; refused %s" % (len(ok), dict(collections.Counter(r["rc"] for r in recs if r["rc"]))))
    print("records that differ %d (sha256 parent %s, tree %s)" % (differ, *(hashlib.sha256(open(o, "rb").read()).hexdigest()[:16] for o in outs)))
    print("kinds with words %s" % {k: sum(1 for r in ok if r["words"][k][0]) for k in KINDS})
    print("engine names (AUTO) %s" % dict(collections.Counter(r["engine_name"] for r in ok if r["engine"] == "AUTO")))
    sam = [r["sampled"] for r in ok if "sampled" in r]
    print("sampled-eligible compiles %d: table learnt %d, refused %s; second learn refused %d; kinds 12 / 13 with words %d / %d" % (
        len(sam), sum(1 for s in sam if s["rc"] == 0), dict(collections.Counter(s["error"][:40] for s in sam if s["rc"])),
        sum(1 for s in sam if s["again"][0] != 0), sum(1 for s in sam if s["words"][0][0]), sum(1 for s in sam if s["words"][1][0])))
    grp = [r for r in every if "group_of" in r]
    print("capture groups %d (of %d patterns): compiled %d, refused %s; kinds 21..24 with words %s" % (
        len(grp), len(set(r["group_of"] for r in grp)), sum(1 for r in grp if r["rc"] == 0),
        dict(collections.Counter(why(r) for r in grp if r["rc"])),
        [sum(1 for r in grp if r["rc"] == 0 and r["words"][k][0]) for k in range(len(GROUP_KINDS))]))
    mul = [r for r in every if "set" in r]
    print("pattern sets %d x forms %d = compiles %d: compiled %d, refused %s; more than one group %s" % (
        len(sets), len(SET_FORMS), len(mul), sum(1 for r in mul if r["rc"] == 0),
        dict(collections.Counter(why(r) for r in mul if r["rc"])),
        {f: sum(1 for r in mul if r["rc"] == 0 and r["form"] == f and len(r["groups"]) > 1) for f in SET_FORMS}))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--as-child":
        child(*sys.argv[2:5])
    else:
        sys.exit(main())
