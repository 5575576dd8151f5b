"""Finished-game records built by hand, word for word as the device loop leaves them in its ring, with the entry the reference
would have dumped for each: what the CPU tests of the game line and of link.records are fed."""
import json
import re

import numpy as np

from ataxxzero_amd.link import RECORD_MAGIC as MAGIC


def cell_name(c):
    return "abcdefg"[c % 7] + "1234567"[c // 7]


def move_name(frm, to):
    return cell_name(to) if frm == to else cell_name(frm) + cell_name(to)


def random_record(rng, plies, visits_hi, random_ply=None, slot=3, uid=77, result=1, zero_total_at=None, targets=None):
    """(record words as the device loop leaves them in its ring, the entry the reference would have dumped)"""
    words = [MAGIC, slot, uid, plies, result, 0, 0 if random_ply is None else random_ply + 1, 0]
    entry = {"boards": [], "dists": [], "moves": [], "result": result}
    if random_ply is not None:
        entry["random_ply"] = random_ply
    for p in range(plies):
        cells = rng.integers(0, 3, size=49)                    # 0 empty, 1 x, 2 o; bit = file + 7 * rank
        x = sum(1 << i for i in range(49) if cells[i] == 1)
        o = sum(1 << i for i in range(49) if cells[i] == 2)
        entry["boards"].append([int(cells[xx + 7 * (6 - y)]) for y in range(7) for xx in range(7)])
        nd = int(rng.integers(0, 40)) if targets is None else targets
        pairs = set()
        while len(pairs) < nd:
            pairs.add((int(rng.integers(0, 49)), int(rng.integers(0, 49))))
        pairs = sorted(pairs)
        rng.shuffle(pairs)
        visits = [int(v) for v in rng.integers(0, visits_hi + 1, size=nd)]
        if zero_total_at == p:
            visits = [0] * nd
        frm, to = (int(rng.integers(0, 49)), int(rng.integers(0, 49))) if not pairs else pairs[0]
        words += [x & 0xFFFFFFFF, x >> 32, o & 0xFFFFFFFF, o >> 32, (frm | to << 8) | nd << 16, 0]
        words += [(f | t << 8) | v << 16 for (f, t), v in zip(pairs, visits)]
        total = sum(visits)
        entry["dists"].append({move_name(f, t): (v / total if total else 0.0) for (f, t), v in zip(pairs, visits)})
        entry["moves"].append(move_name(frm, to))
    words[5] = len(words)
    return np.array(words, dtype=np.uint32), entry


def dumped(entry):
    return json.dumps(entry, sort_keys=True, separators=(",", ":")).encode()


def shortest(line):
    """every double of the line rewritten with its shortest digits (what json.dumps writes); nothing else touched"""
    return re.sub(rb"\d+\.\d+(?:e[-+]\d+)?|\d+e[-+]\d+", lambda m: repr(float(m.group())).encode(), line)


def random_records():
    rng = np.random.default_rng(2026)
    records, entries = [], []
    for case in range(120):
        rec, entry = random_record(rng, plies=int(rng.integers(1, 60)), visits_hi=[1, 7, 100, 400, 800, 2000, 60000][case % 7],
                                   random_ply=int(rng.integers(0, 120)) if case % 5 == 4 else None, result=1 + case % 2,
                                   zero_total_at=0 if case % 11 == 10 else None)
        records.append(rec)
        entries.append(entry)
    return records, entries
