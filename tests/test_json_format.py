"""The game line the host writes for a finished-game record (csrc/json.cpp) — checked on the CPU, no device needed.

The reference's client builds each entry as an nlohmann::json object and writes it with `stream << entry` + newline
(cpp/self_play_client.cpp:512,565-578,637-642): keys sorted, no whitespace, doubles as Grisu2 finds their digits, laid out by
nlohmann's format_buffer (plain decimals between 1e-4 and 1e15, d.ddde-XX outside).  Two independent statements of that:

* the library itself — nlohmann::json 3.1.1 is installed in this image (/opt/conda/include/json.hpp; third party, not part
  of the reference) and oracle/json_entry_dump.cpp builds and streams the entry with it exactly as the reference's code
  does: whole lines must be equal byte for byte (where the header is not installed: equal to the sha256 of the lines it
  wrote, stored in tests/golden/nlohmann_line_digests.json);
* Python's `json.dumps(entry, sort_keys=True, separators=(",", ":"))`: the same bytes except for the one double in a
  thousand that Grisu2 writes with 17 digits where 16 suffice (repr always finds the shortest) — compared with those
  doubles normalised, and value for value.
"""
import ctypes
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from ataxxzero_amd import link
from tests.record_fixtures import MAGIC, dumped, random_record, random_records, shortest


@pytest.mark.parametrize("visits_hi", [1, 7, 400, 2000, 60000])
def test_lines_equal_the_sorted_compact_dump(visits_hi):
    rng = np.random.default_rng(visits_hi)
    for case in range(40):
        rec, entry = random_record(rng, plies=int(rng.integers(1, 30)), visits_hi=visits_hi,
                                   random_ply=int(rng.integers(0, 120)) if case % 4 == 3 else None,
                                   result=1 + case % 2, zero_total_at=0 if case % 10 == 9 else None)
        line = link.format_record_json(rec)
        assert json.loads(line) == entry                     # every value, exactly
        assert shortest(line) == dumped(entry)               # keys, order, separators, integers, lay-out of the doubles
        with_ids = dict(entry, slot=3, uid=77)
        assert shortest(link.format_record_json(rec, with_ids=True)) == dumped(with_ids)


def test_small_ratios_are_written_as_nlohmann_writes_them():
    """1 / 2000 is "0.0005" (not the shorter "5e-04"), 1 / 10000 "0.0001", 1 / 40000 "2.5e-05", 1 / 60000 the
    seventeen-digit form: the boundary of the plain notation is 1e-4, and exponents carry two digits."""
    for total, want in ((2000, b"0.0005"), (10000, b"0.0001"), (40000, b"2.5e-05"), (60000, b"1.6666666666666667e-05"),
                        (3, b"0.3333333333333333"), (1, b"1.0"), (400, b"0.0025")):
        frm, to = 0, 8
        head = [MAGIC, 0, 0, 1, 1, 0, 0, 0]
        ply = [1, 0, 2, 0, (frm | to << 8) | 2 << 16, 0, (frm | to << 8) | 1 << 16, (1 | 9 << 8) | (total - 1) << 16]
        if total == 1:
            ply[4] = (frm | to << 8) | 1 << 16
            ply = ply[:7]
        rec = np.array(head + ply, dtype=np.uint32)
        rec[5] = len(rec)
        line = link.format_record_json(rec)
        assert b'"a1b2":' + want + (b"," if total > 1 else b"}") in line, (total, line)
        assert json.loads(line)["dists"][0]["a1b2"] == 1 / total


def test_malformed_records_are_refused():
    rng = np.random.default_rng(5)
    rec, _ = random_record(rng, plies=4, visits_hi=50)
    bad = rec.copy()
    bad[0] = 0
    with pytest.raises(link.AzhError):
        link.format_record_json(bad)
    with pytest.raises(link.AzhError):
        link.format_record_json(rec[:-1])          # the record says it is longer than what was handed over
    cut = rec.copy()
    cut[3] += 1                                    # one ply more than the words hold
    with pytest.raises(link.AzhError):
        link.format_record_json(cut)
    # the walk the drain's resynchronisation relies on (a payload word may equal the magic): the plies must fill the record
    # exactly, the header fields must be in range, and a dropped game's marker is not a game
    slack = np.concatenate([rec, np.zeros(3, dtype=np.uint32)])
    slack[5] += 3
    with pytest.raises(link.AzhError):
        link.format_record_json(slack)
    odd = rec.copy()
    odd[4] = 7                                     # a result no game has
    with pytest.raises(link.AzhError):
        link.format_record_json(odd)
    marker = np.array([rec[0], 5, 9, 17, 0, 8, 0, 1], dtype=np.uint32)
    with pytest.raises(link.AzhError):
        link.format_record_json(marker)
    # a buffer that is too small reports the size it needs instead of writing a partial line
    need = ctypes.c_int64(0)
    buf = np.zeros(16, dtype=np.uint8)
    rc = link.load().azh_format_record_json(rec.ctypes.data, len(rec), 0, buf.ctypes.data, buf.nbytes, ctypes.byref(need))
    assert rc == -6 and need.value == len(link.format_record_json(rec))


# ------------------------------------------------------------------ against the library the reference itself uses

NLOHMANN = "/opt/conda/include/json.hpp"     # nlohmann::json 3.1.1 ships with this image (third party, not the reference)
# sha256 of every line the library wrote for the record sets below: where the header is not installed the lines are checked
# against these; where it is, the library's own lines must still give them (rewrite: python -m tests.test_json_format)
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nlohmann_line_digests.json")


def digest(line):
    return hashlib.sha256(line).hexdigest()


def visit_ratio_records():
    """n / N for every N <= 800 and every n <= N (the configs' visit counts: 100, 200, 400, 800), two per ply entry, and a
    sample of ratios up to the engine's limit of 60000 visits"""
    head = [MAGIC, 0, 0, 0, 1, 0, 0, 0]
    words, plies = list(head), 0
    records = []

    def flush():
        nonlocal words, plies
        if plies:
            words[3], words[5] = plies, len(words)
            records.append(np.array(words, dtype=np.uint32))
        words, plies = list(head), 0

    rng = np.random.default_rng(7)
    pairs = [(n, N) for N in range(1, 801) for n in range(1, N + 1)]
    pairs += [(int(rng.integers(1, N + 1)), N) for N in rng.integers(801, 60001, size=40000)]
    for n, N in pairs:
        a, b = (0 | 8 << 8), (1 | 9 << 8)                # "a1b2": n, "b1c2": N - n
        ply = [1, 0, 2, 0, a | (2 if N > n else 1) << 16, 0, a | n << 16] + ([b | (N - n) << 16] if N > n else [])
        words += ply
        plies += 1
        if plies == 2000:
            flush()
    flush()
    return records


def build_entry_dump(out_dir):
    """oracle/json_entry_dump.cpp: builds the entry with nlohmann::json exactly as cpp/self_play_client.cpp:512-578 does and
    streams it as :639-641 does -> records -> sha256 of each line it wrote"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(out_dir, "json_entry_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.dirname(NLOHMANN), "-o", exe,
                           os.path.join(root, "oracle", "json_entry_dump.cpp")])

    def run(records):
        out = subprocess.run([exe], input=b"".join(np.ascontiguousarray(r, dtype=np.uint32).tobytes() for r in records),
                             capture_output=True, check=True)
        return [digest(line) for line in out.stdout.split(b"\n")[:-1]]
    return run


@pytest.fixture(scope="module")
def entry_dump(tmp_path_factory):
    """name -> the library's line digests for that record set: from the library where it is installed (and then equal to
    the stored ones), else the stored ones"""
    with open(DIGESTS) as f:
        stored = json.load(f)
    if not os.path.exists(NLOHMANN):
        return lambda name, records: stored[name]
    run = build_entry_dump(str(tmp_path_factory.mktemp("nlohmann")))

    def theirs(name, records):
        lines = run(records)
        assert lines == stored[name], "the installed nlohmann::json writes other lines than the stored digests record"
        return lines
    return theirs


def test_lines_equal_what_nlohmann_json_itself_writes(entry_dump):
    """Byte for byte, including the doubles for which Grisu2 — the library's algorithm — does NOT find the shortest
    digits (json.dumps then differs from the reference, and so did this formatter while it asked std::to_chars)."""
    records, entries = random_records()
    theirs = entry_dump("random_records", records)
    assert len(theirs) == len(records)
    not_shortest = 0
    for rec, entry, their_digest in zip(records, entries, theirs):
        line = link.format_record_json(rec)
        assert digest(line) == their_digest
        assert json.loads(line) == entry                 # same values either way
        not_shortest += line != dumped(entry)
    assert not_shortest > 0, "the sample should hold doubles that Grisu2 writes with 17 digits where 16 suffice"


def test_every_visit_ratio_up_to_800_visits_is_written_as_the_library_writes_it(entry_dump):
    """n / N for every N <= 800 and every n <= N, and a sample of ratios up to 60000 visits (visit_ratio_records)"""
    records = visit_ratio_records()
    theirs = entry_dump("visit_ratio_records", records)
    assert len(theirs) == len(records)
    for rec, their_digest in zip(records, theirs):
        assert digest(link.format_record_json(rec)) == their_digest


def test_formatter_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/json.cpp compiled for the host with ASan + UBSan and driven with 30,000 well-formed and damaged records
    (tests/fuzz/json_fuzz_driver.cpp): no report, damaged records refused, short buffers reported"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "json_fuzz")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(root, "include"),
           "-I" + os.path.join(root, "ataxxzero_amd", "csrc"), "-o", exe,
           os.path.join(root, "tests", "fuzz", "json_fuzz_driver.cpp"), os.path.join(root, "ataxxzero_amd", "csrc", "json.cpp")]
    built = subprocess.run(cmd, capture_output=True)
    if built.returncode != 0:
        pytest.skip("no sanitizer build here: " + built.stderr.decode()[-300:])
    res = subprocess.run([exe, "30000"], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    formatted, refused, small = (int(x) for x in re.findall(rb"\d+", res.stdout))
    assert formatted > 3000 and refused > 3000 and small > 100


if __name__ == "__main__":
    # rewrite tests/golden/nlohmann_line_digests.json from the installed library
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        run = build_entry_dump(tmp)
        with open(DIGESTS, "w") as f:
            json.dump({"random_records": run(random_records()[0]), "visit_ratio_records": run(visit_ratio_records())}, f, indent=0)
            f.write("\n")
