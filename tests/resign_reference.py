"""The recorded search value and the resign rule (azh_engine_set_resign) restated in numpy, for the tests: the ply's value
from the rows of a root report, the rule over per-ply (mover, q bits, counted?), and the decoding of a record's word 5."""
import numpy as np


def ply_value(visits, scores):
    """-> (q as np.float32, visited?) of a root with edge visits `visits` and total scores `scores` (root_report rows):
    q = W_b / n_b of the most visited edge b, ties to the lowest index, one f32 division; 0.5 for a root without a visited
    edge (such a ply neither counts nor resets)."""
    visits = np.asarray(visits, dtype=np.uint32)
    scores = np.asarray(scores, dtype=np.float32)
    if len(visits) == 0 or int(visits.max()) == 0:
        return np.float32(0.5), False
    b = int(np.argmax(visits))            # the first maximum
    with np.errstate(all="ignore"):
        return np.float32(scores[b]) / np.float32(visits[b]), True


def q_bits(q):
    """the 31 bits of q that word 5 keeps"""
    return int(np.array([q], dtype=np.float32).view(np.uint32)[0]) & 0x7FFFFFFF


def q_of_bits(bits):
    return np.array([int(bits) & 0x7FFFFFFF], dtype=np.uint32).view(np.float32)[0]


def decode_word5(word, capped):
    """word 5 of a ply of a record with kind bit 16 -> (q bits, counted?): under the playout cap (kind bit 4) only the FULL
    plies, sign bit set, count.  (A root without a visited edge does not count either; the record cannot tell, and no
    search of at least one visit leaves such a root.)"""
    word = int(word)
    return word & 0x7FFFFFFF, (not capped) or bool(word >> 31)


def replay(plies, q_below, consecutive):
    """The rule over a game's plies [(mover 1 / 2, q bits, counted?)] -> [fired?] per ply: each side has a counter of its
    own consecutive counted plies with q < q_below (the IEEE <: a NaN is never below); a counted ply with q >= q_below
    resets the mover's counter, a ply that does not count leaves it alone; the rule fires at every ply after which the
    mover's counter is >= consecutive (a counter stops at 255)."""
    q_below = np.float32(q_below)
    count = {1: 0, 2: 0}
    fired = []
    for mover, bits, counted in plies:
        hit = False
        if counted:
            count[mover] = min(count[mover] + 1, 255) if bool(q_of_bits(bits) < q_below) else 0
            hit = consecutive > 0 and count[mover] >= consecutive
        fired.append(hit)
    return fired


def first_fire(plies, q_below, consecutive):
    """-> (ply, mover) at which the rule first fires, or None"""
    for p, hit in enumerate(replay(plies, q_below, consecutive)):
        if hit:
            return p, plies[p][0]
    return None
