"""tests/fresh_process.py without a device: the runner in process with plain functions as checks, and the reader against a
throw-away checks module in a child process."""
import json
import os

import pytest

from tests import fresh_process as fp

DEVICE_ERRORS = ["hipMemcpy failed at samples.hip:123: out of memory", "HIP error: invalid device function",
                 "an illegal memory access was encountered"]


def _checks(ran, error=None, measured=None):
    """three checks that say in `ran` that they ran; the second one fails, with `error` or else with an assertion of its own"""
    def check_first():
        ran.append("first")
        if measured is not None:
            measured["check_first"] = 1.5

    def check_second():
        ran.append("second")
        if error is not None:
            raise error
        assert not ran, "the second check's assertion"

    def check_third():
        ran.append("third")
    return [check_first, check_second, check_third]


def _run(tmp_path, checks, **kw):
    path = str(tmp_path / "verdicts.json")
    returned = fp.run(checks, path, prepare=lambda: None, **kw)
    with open(path) as f:
        written = json.load(f)
    assert written == returned
    return written


def test_a_failing_assertion_is_a_traceback_and_the_checks_after_it_run(tmp_path):
    ran = []
    verdicts = _run(tmp_path, _checks(ran))
    assert ran == ["first", "second", "third"]
    assert list(verdicts) == ["check_first", "check_second", "check_third"]
    assert verdicts["check_first"] == verdicts["check_third"] == "ok"
    assert verdicts["check_second"].startswith("Traceback") and "the second check's assertion" in verdicts["check_second"]
    fp.passed(verdicts, "check_third")
    with pytest.raises(AssertionError, match="the second check's assertion"):
        fp.passed(verdicts, "check_second")


def test_only_selects_and_extra_is_kept(tmp_path):
    ran, measured = [], {}
    verdicts = _run(tmp_path, _checks(ran, measured=measured), only=["check_third", "check_first"], extra={"measured": measured})
    assert ran == ["first", "third"]                              # in the order of the list, not of `only`
    assert verdicts == {"measured": {"check_first": 1.5}, "check_first": "ok", "check_third": "ok"}


def test_prepare_runs_first_and_an_empty_selection_still_writes(tmp_path):
    ran = []
    path = str(tmp_path / "verdicts.json")
    fp.run(_checks(ran), path, only=["no_such_check"], prepare=lambda: ran.append("prepare"))
    assert ran == ["prepare"]
    with open(path) as f:
        assert json.load(f) == {}


def test_the_file_is_complete_after_every_check(tmp_path):
    path = str(tmp_path / "verdicts.json")
    snapshots = []

    def look():
        if os.path.exists(path):
            with open(path) as f:
                snapshots.append(list(json.load(f)))
        else:
            snapshots.append(None)

    def check_a():
        look()

    def check_b():
        look()
        raise ValueError("b")

    def check_c():
        look()

    fp.run([check_a, check_b, check_c], path, prepare=lambda: None)
    assert snapshots == [None, ["check_a"], ["check_a", "check_b"]]


@pytest.mark.parametrize("text", DEVICE_ERRORS, ids=["failed-at", "hip-error", "illegal-access"])
def test_a_device_error_ends_the_run(tmp_path, text):
    assert fp.reads_as_device_error(text) and not fp.reads_as_device_error("ok")
    ran = []
    verdicts = _run(tmp_path, _checks(ran, RuntimeError(text)))
    assert ran == ["first", "second"]
    assert list(verdicts) == ["check_first", "check_second"] and text in verdicts["check_second"]
    with pytest.raises(AssertionError, match=r"not run: an earlier check ended in a device error \(check_first, check_second\)"):
        fp.passed(verdicts, "check_third")


def test_an_ordinary_error_does_not_read_as_a_device_error():
    for text in ("hipMemcpy returned 2", "failed at line 3", "an error of the host", "illegal access", "ok"):
        assert not fp.reads_as_device_error(text), text


MODULE = """
import sys
from tests import fresh_process

def check_good():
    print("said by check_good")

def check_bad():
    assert 1 + 1 == 3, "arithmetic"

CHECKS = [check_good, check_bad]

if __name__ == "__main__":
    fresh_process.main(CHECKS, prepare=lambda: None, extra={"argv": sys.argv[2:]})
"""


def test_the_reader_runs_a_checks_module_in_a_child_process(tmp_path, monkeypatch, capsys):
    (tmp_path / "throwaway_checks.py").write_text(MODULE)
    monkeypatch.setenv("PYTHONPATH", os.pathsep.join([str(tmp_path)] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    verdicts = fp.verdicts_of("throwaway_checks", str(tmp_path / "verdicts.json"), timeout=120, echo=True)
    assert "said by check_good" in capsys.readouterr().out
    assert list(verdicts) == ["argv", "check_good", "check_bad"] and verdicts["argv"] == []
    fp.passed(verdicts, "check_good")
    with pytest.raises(AssertionError, match="arithmetic"):
        fp.passed(verdicts, "check_bad")
    with pytest.raises(AssertionError, match="not run"):
        fp.passed(verdicts, "check_missing")
    # a module that does not exist: the return-code assertion, with the child's stderr in it
    with pytest.raises(AssertionError, match="no_such_checks"):
        fp.verdicts_of("no_such_checks", str(tmp_path / "none.json"), timeout=120)
