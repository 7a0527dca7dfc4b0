"""Generate tests/golden/reasm.json: fragment sequences and what the REFERENCE's
own packet_merger (include/seastar/net/packet-util.hh:45-151, built where it
lies through tests/cpp/reasm_ref.cc) holds after every merge: per segment its
offset, length and the crc32 of its bytes.  Needs the reference tree, so it
runs in the build container only; the JSON (data only) travels, and
tests/test_reasm_host.py checks the Python restatement (tests/reasm_model.py)
against it wherever the suite runs.

usage: python tests/golden/make_reasm.py   (deterministic)
"""
import json
import os
import subprocess
import sys
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
REF_INCLUDE = "/root/reference/include"
sys.path.insert(0, TESTS)

import reasm_model  # noqa: E402

SEED, COUNT = 0x4EA53B10, 320


def build_driver(workdir: str) -> str:
    exe = os.path.join(workdir, "reasm_ref")
    cmd = ["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-I", REF_INCLUDE,
           os.path.join(TESTS, "cpp", "reasm_ref.cc"), "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=workdir)
    assert r.returncode == 0, r.stderr
    return exe


def run_driver(exe: str, seqs, workdir: str) -> list:
    """Per sequence, per merge: [(beg, len, bytes), ...] as the reference's merger holds them."""
    cases = os.path.join(workdir, "cases.txt")
    with open(cases, "w") as f:
        for seq in seqs:
            f.write(" ".join([str(len(seq))] + [f"{o} {ln}" for o, ln, _ in seq]) + "\n")
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out, cur = [], None
    for line in r.stdout.splitlines():
        tok = line.split()
        if tok[0] == "S":
            cur = []
            out.append(cur)
            continue
        segs = [(int(tok[1 + 3 * k]), int(tok[2 + 3 * k]), b"" if tok[3 + 3 * k] == "-" else bytes.fromhex(tok[3 + 3 * k]))
                for k in range(int(tok[0]))]
        cur.append(segs)
    assert len(out) == len(seqs) and all(len(o) == len(s) for o, s in zip(out, seqs))
    return out


def main():
    seqs = reasm_model.seeded_sequences(SEED, COUNT)
    with tempfile.TemporaryDirectory() as tmp:
        traces = run_driver(build_driver(tmp), [s for _, s in seqs], tmp)
    doc = {
        "source": "reference build: packet_merger<uint32_t, Tag>::merge of include/seastar/net/packet-util.hh:45-151 "
                  "(tests/cpp/reasm_ref.cc, g++ -std=c++20 -O2); payload byte p of fragment r = "
                  "reasm_model.payload_byte(r, p)",
        "cases": [{"kind": kind, "seq": [list(x) for x in seq],
                   "steps": [[[beg, ln, zlib.crc32(data)] for beg, ln, data in segs] for segs in trace]}
                  for (kind, seq), trace in zip(seqs, traces)],
    }
    with open(os.path.join(HERE, "reasm.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(f"{len(seqs)} sequences -> reasm.json")


if __name__ == "__main__":
    main()
