"""The edge nets of tests/net_edges.py on the CPU: their preconditions (every accumulator order-independent in f32, the
shares of subnormals, ties and non-finite classes each family promises), that every plausible defect of an epilogue or a
matrix unit changes the emulator's result on them — so a kernel with that defect fails tests/test_gpu_net_edges.py —
and the refusal of towers whose numbers are not finite, which azh_net_create decides before it touches a device."""
import numpy as np
import pytest

from ataxxzero_amd import link, model
from oracle import net_oracle
from tests import net_edges as E
from tests import net_exact as ne
from tests.net_compare import classes


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_edge_nets_meet_their_preconditions(case):
    """(edge_net asserts them on the 78 boards under both masks; the shares are repeated here where the issue names them)"""
    family, blocks, filters, fmt = case
    conv, bn, lb, stats = E.edge_net(*case)
    assert len(lb) == 78 and len(conv) == 2 * blocks + 5 and conv[0].shape == (3, 3, 4, filters)
    if family == "small":
        assert min(stats["subnormal_share"]) >= 0.05 and (fmt == "f32" or stats["ties"] >= 20)
    if family == "overflow" and blocks == 0:
        assert min(stats["logit_classes"]) >= 0.05 and stats["boards_all_finite"] >= 1
    if family == "overflow" and blocks > 0:
        assert stats["boards_nan_and_finite"] >= 5 and stats["boards_all_finite"] >= 1


def test_value_nets_walk_the_argument_over_every_kind_of_number():
    """single-piece board k: the argument of tanh is fc_w[cell of k] (fc_b = 0) — zeros of both signs, f32 subnormals,
    2^-20 .. 88, 2^100; with an infinite fc weight +inf, -inf and NaN arguments occur, with a NaN weight only NaNs"""
    single = slice(len(ne.edge_boards()), 78)
    for fmt in E.FORMATS:
        conv, bn, lb, stats = E.edge_net("value-finite", 0, 128, fmt)
        arg = stats["arguments"][:78][single].ravel()
        fc_w = np.asarray(conv[-2], np.float64).ravel()
        assert np.array_equal(np.sort(arg), np.sort(fc_w))            # (a -0 entry arrives as +0: 1 * -0 + 0)
        assert np.signbit(fc_w[fc_w == 0]).any() and not np.signbit(fc_w[fc_w == 0]).all()
        for x in (0.0, 2.0 ** -149, 2.0 ** -20, 0.5, 8.0, float(np.float32(9.1)), 20.0, 88.0, 2.0 ** 100):
            assert (arg == x).any(), x
        for kind, sign in (("pinf", 1), ("ninf", -1)):
            arg = E.edge_net("value-" + kind, 0, 128, fmt)[3]["arguments"]
            assert (arg == np.inf).any() and (arg == -np.inf).any() and np.isnan(arg).any()
            one = E.edge_net("value-" + kind, 0, 128, fmt)[3]["arguments"][:78][single].ravel()
            assert (one == sign * np.inf).any()
        assert np.isnan(E.edge_net("value-nan", 0, 128, fmt)[3]["arguments"]).all()


# defect -> (the families whose nets must see it, the formats it applies to)
DEFECTS = {"relu_erases_nan": (("overflow",), E.FORMATS), "relu_erases_negative_nan_only": (("overflow",), E.FORMATS),
           "flush_subnormal_inputs": (("small",), E.FORMATS), "flush_subnormal_outputs": (("small",), E.FORMATS),
           "saturate_overflow": (("overflow",), E.FORMATS), "truncate": (("small", "large"), ("bf16", "f16"))}


def _differs(a, b):
    return not np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("defect,fmt", [(d, f) for d in sorted(DEFECTS) for f in DEFECTS[d][1]])
def test_every_defect_changes_the_result_on_the_edge_nets(defect, fmt):
    """A kernel whose ReLU erases NaNs (all of them, or those with the sign bit set), whose matrix unit reads subnormal
    operands as zeros, whose conversion flushes subnormal results, saturates instead of overflowing, or truncates,
    computes something else than the emulator — in class or in bits — on EVERY net of the families named above that has a
    layer the defect can act in (the ReLU defects need a block: without one no NaN ever reaches a ReLU)."""
    families = DEFECTS[defect][0]
    seen = 0
    for family, blocks, filters, f in E.TOWER_CASES:
        if f != fmt or family not in families or (defect.startswith("relu") and blocks == 0):
            continue
        conv, bn, lb, _ = E.edge_net(family, blocks, filters, fmt)
        feats = ne.features(lb)
        p, v, _ = net_oracle._forward_lowp(conv, bn, feats, fmt)
        pm, vm, _ = net_oracle._forward_lowp(conv, bn, feats, fmt, defect=defect)
        assert _differs(pm, p) or _differs(vm, v), (defect, family, blocks, filters, fmt)
        if defect.startswith("relu") or defect == "saturate_overflow":
            assert (classes(pm) != classes(p)).any()
        seen += 1
    assert seen >= 3


# ---------------------------------------------------------------- non-finite towers are refused before any device is touched

NAN_POS = np.array([0x7FC00001], np.uint32).view(np.float32)[0]
NAN_NEG = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
BAD = [("nan", NAN_POS), ("negative-nan", NAN_NEG), ("inf", np.float32(np.inf)), ("negative-inf", np.float32(-np.inf))]


def _refused(conv, bn, layer):
    with pytest.raises(link.AzhError) as e:
        link.Net(conv, bn)
    text = str(e.value)
    assert "error -2" in text and "azh_net_create: tower layer %d:" % layer in text and "finite" in text, text


@pytest.mark.parametrize("name,bad", BAD, ids=[b[0] for b in BAD])
def test_a_tower_with_a_number_that_is_not_finite_is_refused(name, bad):
    """a first-layer weight, a block weight and a batch-norm mean: error -2 naming the layer, with or without a GPU
    (the check comes before the device is asked for)"""
    for which, layer in ((0, 0), (2, 2)):
        conv, bn = model.random_init(1, 128, seed=2, perturb_bn=True)
        conv = [np.array(a, np.float32) for a in conv]
        conv[which].reshape(-1)[77] = bad
        _refused(conv, bn, layer)
    conv, bn = model.random_init(1, 128, seed=2, perturb_bn=True)
    bn = [np.array(a, np.float32) for a in bn]
    bn[2][5] = bad                      # the mean of tower layer 1
    _refused(conv, bn, 1)


def test_a_variance_that_gives_no_finite_scale_is_refused():
    """var + eps = 0 (an infinite scale), var + eps < 0 (a NaN), a NaN or infinite variance"""
    for var in (-np.float32(1e-3), np.float32(-1.0), NAN_NEG, NAN_POS):
        conv, bn = model.random_init(1, 128, seed=2, perturb_bn=True)
        bn = [np.array(a, np.float32) for a in bn]
        bn[5][9] = var                  # the variance of tower layer 2
        _refused(conv, bn, 2)
    # an infinite variance gives scale 0: finite, and every weight of the channel folds to 0
    # (the heads stay unrestricted: helpers.nonfinite_net is created by the hostile-evaluation tests)


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_few_positions_of_the_hostile_net_are_too_close_to_call(fmt):
    """helpers.nonfinite_net on the positions of tests/test_hostile_net.py: at most 10 % of them have a deciding
    pre-activation within CLOSE_FACTOR x (the emulator's distance from float64) of zero and are left out of the GPU
    comparison; the rest hold finite, +inf and NaN logits and finite and NaN values"""
    r = E.nonfinite_reference(fmt)
    assert len(r["boards"]) > 150 and r["distance"] > 0 and r["tau"] == E.CLOSE_FACTOR[fmt] * r["distance"]
    assert (~r["keep"]).mean() <= E.MAX_LEFT_OUT, (int((~r["keep"]).sum()), len(r["keep"]))
    p, v = r["p"][r["keep"]], r["v"][r["keep"]]
    assert (classes(p) == 1).any() and (classes(p) == 3).any() and np.isnan(v).sum() >= 30 and np.isfinite(v).sum() >= 30
