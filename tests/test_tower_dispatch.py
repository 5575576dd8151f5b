"""Which tower kernel a launch runs.  The library has one dispatch function; azh_net_tower_choice asks it without a launch
and without a device.  Here the decision list is restated and held against it over every combination of its inputs, so that
a change which loses the thin flag, or falls back to the 32x32 tower, fails a test instead of showing up as a slower bench."""
import itertools

from ataxxzero_amd import link

NAMES = {link.DTYPE_F32: "f32", link.DTYPE_BF16: "bf16", link.DTYPE_F16: "f16"}
FLAGS = list(itertools.product([False, True], repeat=5))     # thin, stamped, variant1, six, range_ok


def k_tower(dt, nb, wps, stamp=False, ft=128):
    """k_tower<DT,NB,WPS,STAMP,FT>: a wave per 32 channels, __launch_bounds__(threads, WPS)"""
    args = [NAMES[dt], str(nb), str(wps)] + (["true" if stamp else "false"] if stamp or ft != 128 else []) + ([str(ft)] if ft != 128 else [])
    threads = 64 * ft // 32
    return 0, dict(kernel="k_tower<%s>" % ",".join(args), boards=nb, threads=threads, per_cu=max(1, wps * 256 // threads))


def k_tower2(name, boards, *args):
    """the variant 2 kernels: 256 threads, two workgroups per CU"""
    return 0, dict(kernel="%s<%s>" % (name, ",".join(args)), boards=boards, threads=256, per_cu=2)


def restated(filters, dt, thin, stamped, variant1, six, range_ok):
    bits16 = dt != link.DTYPE_F32
    if filters != 128:
        if stamped:
            return -2, None
        return k_tower(dt, 3, 1, ft=64) if filters == 64 else k_tower(dt, 3 if bits16 else 1, 2, ft=256)
    if bits16 and not variant1 and range_ok:
        if stamped:
            return k_tower2("k_tower2", 3, "bf16", "true") if dt == link.DTYPE_BF16 else (-2, None)
        return k_tower2("k_tower2_thin", 1, NAMES[dt]) if thin else k_tower2("k_tower2", 3, NAMES[dt])
    if stamped and dt != link.DTYPE_BF16:
        return -2, None
    if not bits16:
        return k_tower(dt, 3, 1)
    return k_tower(dt, 6, 1, stamped) if six else k_tower(dt, 3, 2, stamped)


def restated_pair(filters, dt, thin, variant1, range_ok):
    if dt == link.DTYPE_F32 or filters != 128 or variant1 or not range_ok:
        return 1, None
    return k_tower2("k_tower2_pair", 1, NAMES[dt], "Geo2Thin") if thin else k_tower2("k_tower2_pair", 3, NAMES[dt])


def _same(got, want, what):
    rc, row = got
    assert rc == want[0], what
    assert (row is None) == (want[1] is None), what
    if row:
        assert {k: row[k] for k in want[1]} == want[1], what
        assert 0 < row["lds_bytes"] <= 160 * 1024, what
    return row


def test_every_launch_runs_the_kernel_of_the_restated_decision_list():
    seen = set()
    for filters, dt, (thin, stamped, variant1, six, range_ok) in itertools.product([64, 128, 256], NAMES, FLAGS):
        what = (filters, NAMES[dt], thin, stamped, variant1, six, range_ok)
        row = _same(link.tower_choice(filters, dt, thin, stamped, False, variant1, six, range_ok),
                    restated(filters, dt, thin, stamped, variant1, six, range_ok), what)
        seen.add(row["kernel"] if row else None)
    for filters, dt, (thin, _, variant1, six, range_ok) in itertools.product([64, 128, 256], NAMES, FLAGS):
        what = ("pair", filters, NAMES[dt], thin, variant1, six, range_ok)
        row = _same(link.tower_choice(filters, dt, thin, False, True, variant1, six, range_ok),
                    restated_pair(filters, dt, thin, variant1, range_ok), what)
        seen.add(row["kernel"] if row else None)
    assert len(seen - {None}) == 22, sorted(seen - {None})


def test_thin_and_three_board_rows_of_variant_2_ask_for_the_same_lds():
    for dt in (link.DTYPE_BF16, link.DTYPE_F16):
        for pair in (False, True):
            (_, thin), (_, three) = (link.tower_choice(128, dt, thin=t, pair=pair) for t in (True, False))
            assert thin["kernel"] != three["kernel"] and thin["boards"] == 1 and three["boards"] == 3
            assert thin["lds_bytes"] == three["lds_bytes"]


def test_defaults_are_the_flagship_kernel():
    assert link.tower_choice(128, link.DTYPE_BF16)[1]["kernel"] == "k_tower2<bf16>"
