"""bench.py --dump-outputs: the accept bitmap of the last timed step is written exactly (uint32 words as float64), and a
bitmap beyond the size cap as a fixed, seeded sample of its words with their indices.  The writer on the CPU; a plain run of
bench.py on the GPU, its dump against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_bitmap_is_written_whole_and_exact(tmp_path):
    bits = np.random.default_rng(3).integers(0, 1 << 32, size=1000, dtype=np.uint64).astype(np.uint32)
    bits[:3] = (0, 0xFFFFFFFF, 0x80000001)
    (tmp_path / "accept_bits_index.npy").write_bytes(b"stale")          # left by an earlier, sampled dump
    bench.dump_outputs(str(tmp_path), bits)
    got = np.load(tmp_path / "accept_bits.npy")
    assert got.dtype == np.float64 and (got.astype(np.uint64) == bits).all()
    assert not (tmp_path / "accept_bits_index.npy").exists()


def test_large_bitmap_is_a_seeded_sample_within_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096 + 16 * 500)
    bits = np.arange(100_000, dtype=np.uint32) * np.uint32(2654435761)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), bits)
    vals, idx = (np.load(tmp_path / "a" / n) for n in ("accept_bits.npy", "accept_bits_index.npy"))
    assert vals.dtype == idx.dtype == np.float64 and vals.size == idx.size == 500
    assert (np.diff(idx) > 0).all() and (vals.astype(np.uint64) == bits[idx.astype(np.int64)]).all()
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")) <= bench.DUMP_BYTES
    assert (np.load(tmp_path / "b" / "accept_bits_index.npy") == idx).all()                  # the same sample every run


@pytest.mark.gpu
def test_plain_run_dumps_the_bitmap_of_the_oracle(tmp_path):
    """bench.py in a process of its own on 8 MiB of the email config: the dumped bitmap is the oracle's accept vector packed
    32 lines to a word (the slice, the uint32 view and the moment of the dump at the call site), and the plain run timed
    exactly --steps launches and left the --full figures out."""
    nbytes = 8 << 20
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "email", "--bytes", str(nbytes),
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]
    assert res["steps"] == 3 and len(res["roofline"]["kernel_ms_each_launch"]) == 3 and res["ms_per_step"] > 0
    assert "cold" not in res and "cpu_baseline" not in res and res["config"]["accepted_rank0"] is None

    import synth
    from pyoracle import OracleRegex
    kind, pkey = bench.WORKLOADS["email"][:2]
    host = np.empty(nbytes, dtype=np.uint8)
    synth.fill(kind, 2, host)
    want = OracleRegex(bench.patterns()[pkey]).match_lines(host)
    packed = np.packbits(want.astype(bool), bitorder="little")
    words = np.zeros((len(want) + 31) // 32 * 4, dtype=np.uint8)
    words[:packed.size] = packed
    got = np.load(tmp_path / "accept_bits.npy")
    assert res["config"]["lines_per_gpu"] == len(want) and got.dtype == np.float64
    assert np.array_equal(got.astype(np.uint32), words.view("<u4"))
    assert not (tmp_path / "accept_bits_index.npy").exists()
