"""train.py --prove-depth without a GPU: the alpha-beta limits are checked, each with the limit named, before anything touches
the device (the games file named here does not even exist), by the command line and by the library call; and the flags' help
and defaults."""
import os
import subprocess
import sys

import pytest

from ataxxzero_amd import link, training

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REFUSALS = [(["--prove-depth", "9"], "--prove-depth must be 1 .. 8"),
            (["--prove-depth", "-1"], "--prove-depth must be 1 .. 8"),
            (["--prove-depth", "4"], "--prove-nodes 0 (no limit) is accepted up to --prove-depth 3 only"),
            (["--prove-depth", "3", "--prove-nodes", "100"], "--prove-nodes must be 0 (no limit) or at least 256"),
            (["--prove-depth", "8", "--prove-nodes", "255"], "--prove-nodes must be 0 (no limit) or at least 256"),
            (["--prove-nodes", "4096"], "need --prove-depth"),
            (["--prove-policy"], "need --prove-depth")]


@pytest.mark.parametrize("flags, message", REFUSALS)
def test_train_cli_refusals(flags, message, tmp_path):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--games", str(tmp_path / "none.json"), "--new-path",
                          str(tmp_path / "new.npy")] + flags, cwd=ROOT, capture_output=True, timeout=300)
    assert res.returncode != 0 and not os.path.exists(str(tmp_path / "new.npy"))
    err = res.stderr.decode()
    assert "train.py: " + message in err or message in err, err[-2000:]
    assert "Traceback" not in err and "Found" not in res.stdout.decode()    # refused before the games were even opened


def test_the_limits_are_the_searchs():
    assert (link.ALPHABETA_MAX_DEPTH, link.ALPHABETA_UNBOUNDED_DEPTH, link.MAX_MOVES) == (8, 3, 256)
    for depth in range(1, 9):
        assert training.prove_refusal(depth, 256) is None and training.prove_refusal(depth, 1 << 40) is None
        assert (training.prove_refusal(depth, 0) is None) == (depth <= 3)
        assert "at least 256" in training.prove_refusal(depth, 255)
    assert "1 .. 8" in training.prove_refusal(0, 0) and "1 .. 8" in training.prove_refusal(9, 4096)


@pytest.mark.parametrize("kwargs, message", [({"prove_depth": 9}, "1 .. 8"), ({"prove_depth": 4}, "up to --prove-depth 3"),
                                             ({"prove_depth": 3, "prove_nodes": 100}, "at least 256"),
                                             ({"prove_nodes": 4096}, "need --prove-depth"),
                                             ({"prove_policy": True}, "need --prove-depth")])
def test_train_refuses_in_the_library_call_too(kwargs, message, tmp_path):
    with pytest.raises(ValueError, match=message):                          # before the games file is opened
        training.train([str(tmp_path / "none.json")], None, str(tmp_path / "new.npy"), steps=1, **kwargs)


def test_the_flags_are_off_by_default_and_documented():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--help"], cwd=ROOT, capture_output=True, timeout=300)
    text = res.stdout.decode()
    assert res.returncode == 0
    for flag in ("--prove-depth", "--prove-nodes", "--prove-policy"):
        assert flag in text, flag
