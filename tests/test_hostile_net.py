"""helpers.nonfinite_net on the CPU (oracle.net_oracle.forward, float64): over the positions of random lines from the late start
position both finite and non-finite values occur, and rows with and without a +inf logit at a legal move — so a device loop
fed by it meets non-finite evaluations and ordinary ones (tests/test_gpu_hostile_evals.py).  And helpers.HostileEvaluator
writes the bits it says."""
import numpy as np

from oracle import net_oracle
from tests import helpers
from tests.engine_harness import late_start_fen


def test_the_net_gives_finite_and_non_finite_evaluations():
    boards = []
    for seed in range(12):
        for packed, _, _ in helpers.random_line(late_start_fen(), seed):
            w0, w1 = int(packed[0]), int(packed[1])
            x = w0 & ~(1 << 63)
            boards.append((w1, x) if w0 >> 63 else (x, w1))
    boards = np.array(boards, dtype=np.uint64)
    assert len(boards) > 150
    conv, bn = helpers.nonfinite_net()
    with np.errstate(all="ignore"):
        pol, val = net_oracle.forward(conv, bn, net_oracle.features_from_leaf_boards(boards, 0))
    pol, val = pol.reshape(len(boards), 833), val.reshape(-1)
    nan_values = int(np.isnan(val).sum())
    assert nan_values >= 30 and len(val) - nan_values >= 30 and (np.abs(val[~np.isnan(val)]) == 1.0).all()
    hit = sum(int(np.isposinf(pol[i, helpers.legal_policy_indices(b)]).any()) for i, b in enumerate(boards))
    assert hit >= 30 and len(boards) - hit >= 30
    finite_layers = np.isfinite(pol.reshape(-1, 49, 17)[:, :, :16]).all()
    assert finite_layers and not np.isfinite(pol.reshape(-1, 49, 17)[:, :, 16]).any()


def test_the_hostile_evaluator_writes_the_bits_it_names():
    lb = np.array([[0x0000000000000041, 0x0001000000000000], [0x1F, 0x3E0]], dtype=np.uint64)
    base_l, base_v = helpers.synthetic_evals_distinct(lb)
    table = {"a": [("row_nan", True), ("value_nan", False)], "b": [("row_spike", False), ("value_minus1", False)],
             "c": [("row_inf3", False), ("row_part_nan", False), ("value_ninf", False)]}
    ev = helpers.HostileEvaluator(lambda key: table[key])
    l, v = ev(lb, ["a", None])
    assert (l.view(np.uint32)[0] == 0xFFC00001).all() and v.view(np.uint32)[0] == 0x7FC00001
    assert (l[1] == base_l[1]).all() and v[1] == base_v[1]
    l, v = ev(lb, ["b", "c"], counted=[True, False])
    legal = helpers.legal_policy_indices(lb[0])
    assert len(legal) > 1 and l[0, legal[-1]] == np.float32(1e30) and (np.delete(l[0], legal[-1]) == np.delete(base_l[0], legal[-1])).all()
    assert v[0] == -1.0 and np.isneginf(v[1])
    assert np.isposinf(l[1, 0:100:3]).all() and (l.view(np.uint32)[1, 100:300] == 0x7FC00001).all() and np.isposinf(l[1, 300::3]).all()
    assert ev.seen == {("row_nan", True): 1, ("value_nan", False): 1, ("row_spike", False): 1, ("value_minus1", False): 1}
