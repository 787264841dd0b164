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
outputs, a second rrx_learn_table's refusal, and the kinds 12 and 13 again."""
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

    def words(h, kind):
        n = L.rrx_program_words(h, kind, None, 0)
        buf = (C.c_uint32 * max(n, 1))()
        L.rrx_program_words(h, kind, buf, n)
        return [n, hashlib.sha256(bytes(buf)[:4 * n]).hexdigest()]

    pats = json.load(open(pattern_file))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=2)
    ap.add_argument("--random", type=int, default=2000)
    ap.add_argument("--out", default=os.environ.get("PROBE_OUT", os.path.join(ROOT, "probe_out")))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    pats = pattern_set(a.random)
    pfile = os.path.join(a.out, "equivalence_patterns.json")
    json.dump(pats, open(pfile, "w"))
    outs = [os.path.join(a.out, "equivalence_%s.jsonl" % side) for side in ("parent", "tree")]
    kids = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--as-child", lib, pfile, o]) for lib, o in zip(a.libs, outs)]
    assert all(k.wait() == 0 for k in kids), "a child failed"
    A, B = (open(o).read().splitlines() for o in outs)
    differ = sum(x != y for x, y in zip(A, B)) + abs(len(A) - len(B))
    recs = [json.loads(x) for x in B]
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
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--as-child":
        child(*sys.argv[2:5])
    else:
        sys.exit(main())
