"""Every tower kernel that azh_net_forward can reach, at the edges of bf16, f16 and f32, against the emulator
(oracle.net_oracle.forward_lowp) by the class-aware rule of tests/net_compare.py: the same NaN, +inf and -inf positions,
every finite logit bit for bit, every finite value within 4 f32 ulp of the float64 tanh, +-1 for an infinite argument.

The nets are the hand-built exact nets of tests/net_edges.py (subnormals and their ties, the largest finite values,
overflow from finite weights, a value head over every kind of argument); their preconditions are checked on the CPU by
tests/test_net_edges_host.py, where each plausible defect of an epilogue is also shown to change the result on them.
Kernels: k_tower2 and k_tower2_thin (16 bits, 128 filters), k_tower (f32; 64 filters; and, in two fresh child processes,
AZH_TOWER=1 with three and with six boards per workgroup), k_sym_reduce.  k_tower2_pair is reachable only through the
engine and shares its layer epilogue (AZH_LAYER_EPILOGUE2) with k_tower2: it is left out here.

What the MI355X did when these tests were written (gfx950, ROCm 7): see DESIGN.md, "Towers at the edges of their formats"."""
import numpy as np
import pytest

from ataxxzero_amd import link, model
from oracle import net_oracle
from tests import helpers
from tests import net_edges as E
from tests import net_exact as ne
from tests.net_compare import assert_equals_emulator, classes, run_forward_jobs, same_classes

pytestmark = pytest.mark.gpu

DT = {"f32": link.DTYPE_F32, "bf16": link.DTYPE_BF16, "f16": link.DTYPE_F16}
BATCHES = (1, 2, 4, 7, None)          # boards per launch (None: all 78): partial workgroups of 3 and of 6


def _selection(k, n):
    """k boards spread over the n of the case, so that a small batch is not just the empty and the full board"""
    return np.arange(n) if k is None else (np.arange(k) * 11 + 3) % n


# The bf16 16x16x32 towers (k_tower2, k_tower2_thin) take relu as a packed integer max with 0 on the converted pair, which clears
# the NaN this device generates (0xFFC00000, sign bit set): after a block an overflowed activation is 0 there and a NaN in the
# emulator — e.g. 459 of the 833 logits of one board of the 1-block net, 765 of 833 of the 2-block net (NaN -> finite).  The
# NaN-keeping epilogue (v_maximum3_f32 before the conversion) was measured against the parent in one session, bench.py's
# headline in node-evals/s: parent 4,479,542 and 4,473,005 (its own spread 0.15 %), with the fix 4,448,351 and 4,467,442
# (-0.70 % and -0.12 %) — not within the spread, so bf16 stays as it was.  f16 is fixed (v_pk_maximum3_f16, the
# same instruction count).  strict: the day bf16 keeps its NaNs these marks must go.  What the bf16 towers compute instead is
# pinned bit for bit by test_bf16_towers_clear_the_generated_nan_and_nothing_else below, so the marks hide nothing else.
BF16_RELU = pytest.mark.xfail(strict=True, reason="bf16 k_tower2: the packed integer relu clears the device's NaN (sign bit set)")


def _marked(case):
    family, blocks, filters, fmt = case
    bad = family == "overflow" and blocks > 0 and filters == 128 and fmt == "bf16"
    return pytest.param(case, id=E.case_id(case), marks=[BF16_RELU] if bad else [])


@pytest.mark.parametrize("case", [_marked(c) for c in E.CASES])
def test_tower_equals_the_emulator_at_the_edges(case):
    """in process: f32, bf16 and f16 on k_tower2, thin=True (k_tower2_thin), the 64-filter nets on k_tower; both masks"""
    family, blocks, filters, fmt = case
    conv, bn, lb, _ = E.edge_net(*case)
    net = link.Net(conv, bn)
    for mask in ne.MASKS:
        ref_p, ref_v, ref_arg = E.reference(*case, mask)
        for k in BATCHES:
            sel = _selection(k, len(lb))
            for thin in ((False, True) if fmt != "f32" and filters == 128 else (False,)):
                p, v = net.forward(lb[sel], mask, DT[fmt], thin=thin)
                what = "%s mask %#x, %d boards, thin=%s" % (E.case_id(case), mask, len(sel), thin)
                if family == "overflow" and k is None and mask == ne.MASKS[0]:
                    nan = p.view(np.uint32)[np.isnan(p)]
                    helpers.note("%s: %d NaN logits, sign bit set in %d, patterns %s" % (what, nan.size, (nan >> 31).sum(),
                                                                                       sorted("%#x" % x for x in set(nan.tolist()))[:4]))
                assert_equals_emulator(p, v, ref_p[sel], ref_v[sel], what, ref_arg=ref_arg[sel])
    net.close()


@pytest.mark.parametrize("blocks", [1, 2])
def test_bf16_towers_clear_the_generated_nan_and_nothing_else(blocks):
    """The cases marked above, against the emulator with the one defect the bf16 16x16x32 towers are known to have
    (relu_erases_negative_nan_only: the ReLU clears a NaN whose sign bit is set, and the device's is): k_tower2 and
    k_tower2_thin equal it class for class and bit for bit, under both masks and every batch size — any other difference
    from the emulator on these nets fails here.  (The order independence of the changed accumulators is checked on the CPU
    by net_edges.reference_erased_nan.)"""
    case = ("overflow", blocks, 128, "bf16")
    conv, bn, lb, _ = E.edge_net(*case)
    net = link.Net(conv, bn)
    for mask in ne.MASKS:
        ref_p, ref_v, ref_arg = E.reference_erased_nan(*case, mask)
        faithful_p = E.reference(*case, mask)[0]
        assert (classes(ref_p) != classes(faithful_p)).any() and np.isinf(E.trace(conv, bn, ne.features(lb[:8]), "bf16")[0]["a"]).any()
        for k in BATCHES:
            sel = _selection(k, len(lb))
            for thin in (False, True):
                p, v = net.forward(lb[sel], mask, DT["bf16"], thin=thin)
                assert_equals_emulator(p, v, ref_p[sel], ref_v[sel], "%s with the NaN-clearing ReLU, mask %#x, %d boards, thin=%s"
                                       % (E.case_id(case), mask, len(sel), thin), ref_arg=ref_arg[sel])
    net.close()


@pytest.mark.parametrize("env", [{"AZH_TOWER": "1"}, {"AZH_TOWER": "1", "AZH_TOWER_BOARDS": "6"}],
                         ids=["variant1-3boards", "variant1-6boards"])
def test_variant1_towers_equal_the_emulator_at_the_edges(env, tmp_path):
    """k_tower<DT,3,2> and k_tower<DT,6,1> at 128 filters — also the fallback on a device whose out-of-range LDS reads do
    not return zeros — in a fresh process each: every 16-bit edge net of 128 filters, both masks, partial workgroups"""
    jobs, refs = {}, {}
    for case in [c for c in E.CASES if c[2] == 128 and c[3] != "f32"]:
        conv, bn, lb, _ = E.edge_net(*case)
        weights = str(tmp_path / (E.case_id(case) + ".npy"))
        model.save_model(weights, conv, bn)
        for mask in ne.MASKS:
            ref_p, ref_v, ref_arg = E.reference(*case, mask)
            for k in BATCHES:
                sel = _selection(k, len(lb))
                name = "%s-%x-%d" % (E.case_id(case), mask, len(sel))
                jobs[name] = (weights, lb[sel], mask, DT[case[3]], 0)
                refs[name] = (ref_p[sel], ref_v[sel], ref_arg[sel])
    got = run_forward_jobs(jobs, env, tmp_path)
    for name, (ref_p, ref_v, ref_arg) in refs.items():
        assert_equals_emulator(got[name + "_p"], got[name + "_v"], ref_p, ref_v, "%s %s" % (env, name), ref_arg=ref_arg)


def test_symmetry_average_of_an_overflowing_net_by_class():
    """AZH_FORWARD_SYM on the one-block f16 overflow net: k_sym_reduce is the mean of eight, so a logit is a NaN if any of
    its eight images is one (or if +inf and -inf meet), and the classes equal forward_lowp_sym's"""
    case = ("overflow", 1, 128, "f16")
    conv, bn, lb, _ = E.edge_net(*case)
    lb = lb[_selection(16, len(lb))]
    net = link.Net(conv, bn)
    for mask in ne.MASKS:
        with np.errstate(invalid="ignore", over="ignore"):
            ref_p, ref_v = net_oracle.forward_lowp_sym(conv, bn, net_oracle.features_from_leaf_boards(lb, mask), "f16")
        p, v = net.forward_sym(lb, mask, DT["f16"])
        cls = same_classes(p, ref_p.astype(np.float32), "sym logits mask %#x" % mask)
        same_classes(v.ravel(), ref_v.ravel(), "sym values mask %#x" % mask)
        assert (cls == 3).any() and (cls == 0).any()
    net.close()


@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32"])
def test_finite_boards_between_overflowing_neighbours(fmt):
    """One net, finite on boards without a piece of the mover and overflowing on the others: the finite boards' logits and
    values are bit-identical whether they are launched alone or between overflowing boards, in every slot of a 3-board
    workgroup (and of a 6-board one's first half).  That the neighbours overflow is the emulator's statement (their first
    layer holds infinities, their logits NaNs); on the device their logits hold NaNs too, except in the bf16 16x16x32 towers,
    whose ReLU clears them (BF16_RELU above) — the property asked of the finite boards is the same there."""
    conv, bn, lb, _ = E.edge_net("overflow", 1, 128, fmt)
    rng = np.random.default_rng(11)
    quiet = np.array([(0, sum(1 << int(c) for c in rng.permutation(49)[:k])) for k in (0, 1, 5, 20, 30, 48)], dtype=np.uint64)
    loud = lb[[1, 2, 6, 10, 40, 60]]
    net = link.Net(conv, bn)
    mask = ne.ASYM_BLOCKERS
    alone_p, alone_v = net.forward(quiet, mask, DT[fmt])
    assert np.isfinite(alone_p).all() and np.isfinite(alone_v).all() and np.unique(alone_p).size > 100
    loud_feats = net_oracle.features_from_leaf_boards(loud, mask)
    assert all(np.isinf(a).any() for a in E.trace(conv, bn, loud_feats, fmt)[0]["a"])
    assert all(np.isnan(b).any() for b in net_oracle.forward_lowp(conv, bn, loud_feats, fmt)[0])
    if fmt != "bf16":
        loud_p, _ = net.forward(loud, mask, DT[fmt])
        assert all(np.isnan(b).any() for b in loud_p)
    for slot in range(3):
        batch, where = [], []
        for i, q in enumerate(quiet):
            group = [loud[(2 * i) % len(loud)], loud[(2 * i + 1) % len(loud)]]
            group.insert(slot, q)
            where.append(len(batch) + slot)
            batch += group
        batch = np.array(batch, dtype=np.uint64)
        for thin in ((False, True) if fmt != "f32" else (False,)):
            p, v = net.forward(batch, mask, DT[fmt], thin=thin)
            assert (p[where].view(np.uint32) == alone_p.view(np.uint32)).all(), (fmt, slot, thin)
            assert (v[where].view(np.uint32) == alone_v.view(np.uint32)).all(), (fmt, slot, thin)
    net.close()


# finite entries: the bounds of test_gpu_net.py's test_reduced_precision_tower_tracks_f32 for the 16-bit towers (there
# against the f32 tower, here against the emulator of the same dtype); the f32 tower within the f32 path's 1e-5 gate
HOSTILE_TOL = {"bf16": 2e-3, "f16": 3e-4, "f32": 1e-5}


@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32"])
def test_the_hostile_net_has_the_emulators_classes(fmt):
    """helpers.nonfinite_net — the net the hostile-evaluation tests trust, infinite weights in its heads — on the positions
    of tests/test_hostile_net.py: the NaN and +-inf positions of logits and values are forward_lowp's, the finite entries
    within HOSTILE_TOL; left out are the positions with a deciding pre-activation too close to zero for a random net
    (tests/net_edges.py, nonfinite_reference: threshold, reasoning, and the 10 % cap checked on the CPU)."""
    r = E.nonfinite_reference(fmt)
    keep = r["keep"]
    assert (~keep).mean() <= E.MAX_LEFT_OUT
    net = link.Net(*helpers.nonfinite_net())
    helpers.note("hostile net %s: %d of %d positions left out (|z| < %.3e = %g x the emulator's distance %.3e from float64)"
                 % (fmt, (~keep).sum(), len(keep), r["tau"], r["factor"], r["distance"]))
    for thin in ((False, True) if fmt != "f32" else (False,)):
        p, v = net.forward(r["boards"], 0, DT[fmt], thin=thin)
        p, v, ref_p, ref_v = p[keep], v[keep].ravel(), r["p"][keep], r["v"][keep].ravel()
        fin = same_classes(p, ref_p.astype(np.float32), "hostile net %s thin=%s: logits" % (fmt, thin)) == 0
        assert np.abs(p[fin] - ref_p[fin]).max() <= HOSTILE_TOL[fmt]
        fin = same_classes(v, ref_v, "hostile net %s thin=%s: values" % (fmt, thin)) == 0
        assert np.abs(v[fin] - ref_v[fin]).max() <= HOSTILE_TOL[fmt]
    net.close()


def test_a_weight_that_overflows_in_f16_is_refused_for_f16_only():
    """70000 is a finite f32 and bf16 number and an infinite f16: azh_net_forward returns -2 for f16 and launches nothing
    (the outputs keep their initial zeros), and the same net object goes on serving f32 and bf16"""
    conv, bn = model.random_init(1, 128, seed=2)
    conv = [np.array(a, np.float32) for a in conv]
    scale = net_oracle.bn_constants(bn[2], bn[3])[0]
    conv[1][1, 1, 7, 9] = np.float32(70000.0) / scale[9]
    assert np.isinf(net_oracle.round_f16(conv[1] * scale)).any() and np.isfinite(net_oracle.round_bf16(conv[1] * scale)).all()
    net = link.Net(conv, bn)
    lb = ne.edge_boards()[:7]
    f32_p, _ = net.forward(lb, 0, link.DTYPE_F32)
    for again in range(2):
        with pytest.raises(link.AzhError) as e:
            net.forward(lb, 0, link.DTYPE_F16)
        assert "error -2" in str(e.value) and "tower layer 1" in str(e.value) and "finite" in str(e.value)
        with pytest.raises(link.AzhError):
            net.forward(lb, 0, link.DTYPE_F16, thin=True)
        p, v = net.forward(lb, 0, link.DTYPE_BF16)
        assert np.isfinite(p).all() and np.isfinite(v).all() and np.abs(p).max() > 0
        p, v = net.forward(lb, 0, link.DTYPE_F32)
        assert (p == f32_p).all()
    net.close()


def test_the_engine_passes_the_refusal_of_a_dtype_on():
    """The same net through the engine's own launches (azh_engine_run -> azh_net_launch, and the arena's two-net launch,
    azh_net_launch_pair, with the refused net on either side): error -2 naming the layer for f16; bf16 runs."""
    conv, bn = model.random_init(1, 128, seed=2)
    conv = [np.array(a, np.float32) for a in conv]
    conv[1][1, 1, 7, 9] = np.float32(70000.0) / net_oracle.bn_constants(bn[2], bn[3])[0][9]
    bad, good = link.Net(conv, bn), link.Net(*model.random_init(1, 128, seed=3))
    from oracle import oracle_lib as orc
    for flags, runs in ((0, [lambda e, dt: e.run(bad, 3, dt)]),
                        (orc.FLAG_ARENA, [lambda e, dt: e.run_arena(bad, good, 3, dt), lambda e, dt: e.run_arena(good, bad, 3, dt)])):
        ocfg = orc.make_config(games=32, visits=8, seed=1, weight=0.0, flags=flags)
        for run in runs:
            for dtype in (link.DTYPE_F16, link.DTYPE_BF16):      # (a fresh engine each: a refused run stops after its select)
                engine = link.Engine(link.Config(**{n: getattr(ocfg, n) for n, _ in orc.Config._fields_}))
                if dtype == link.DTYPE_F16:
                    with pytest.raises(link.AzhError) as e:
                        run(engine, dtype)
                    assert "error -2" in str(e.value) and "tower layer 1" in str(e.value), str(e.value)
                else:
                    run(engine, dtype)
                engine.sync()
                assert sum(engine.game_state(g).ply for g in range(32)) == 0
                engine.close()
    bad.close()
    good.close()
