"""What "a tower equals the emulator" means, in one place, and the fresh child process that runs a list of forward jobs
under another tower variant.  Shared by tests/test_gpu_net_exact.py, tests/test_gpu_net_edges.py and tests/test_gpu_net.py.

The rule (class-aware; on all-finite results it is the rule test_gpu_net_exact.py has always applied):
  * the NaN positions are the same — a NaN is a NaN whatever its sign and payload;
  * the +inf and the -inf positions are the same;
  * every finite logit is bit-equal, zeros of either sign counting as equal;
  * every finite value is within 4 f32 ulp of the float64 tanh of the emulator's f32 argument (or within value_tol);
  * where the argument is +-inf the value is exactly +-1."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASS_NAMES = ("finite", "+inf", "-inf", "NaN")


def classes(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    x = np.asarray(x)
    return np.where(np.isnan(x), 3, np.where(x == np.inf, 1, np.where(x == -np.inf, 2, 0)))


def same_classes(got, ref, what):
    cg, cr = classes(got), classes(ref)
    bad = cg != cr
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        pairs = sorted({(CLASS_NAMES[a], CLASS_NAMES[b]) for a, b in zip(cr[bad].ravel(), cg[bad].ravel())})
        raise AssertionError("%s: %d of %d entries differ in class (emulator -> kernel: %s); first at %s: kernel %r, emulator %r"
                             % (what, bad.sum(), bad.size, pairs, i, float(np.asarray(got)[i]), float(np.asarray(ref)[i])))
    return cr


def assert_equals_emulator(p, v, ref_p, ref_v, what, value_tol=None, ref_arg=None):
    """p, v: a tower's logits and values (f32); ref_p, ref_v: forward_lowp's (float64: f32 logits, the float64 tanh);
    ref_arg: the emulator's f32 argument of tanh, where the +-1 of an infinite argument is to be checked"""
    with np.errstate(invalid="ignore", over="ignore"):
        ref32 = np.asarray(ref_p).astype(np.float32)
    finite = same_classes(p, ref32, what + ": logits") == 0
    bad = finite & (p != ref32)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d finite logits differ; first at %s: kernel %r, emulator %r"
                             % (what, bad.sum(), finite.sum(), i, float(p[i]), float(ref32[i])))
    v, ref_v = np.asarray(v).reshape(-1), np.asarray(ref_v, np.float64).reshape(-1)
    finite = same_classes(v, ref_v, what + ": values") == 0
    tol = value_tol if value_tol is not None else 4 * np.spacing(np.abs(ref_v[finite]).astype(np.float32)).astype(np.float64)
    dv = np.abs(v[finite].astype(np.float64) - ref_v[finite])
    assert (dv <= tol).all(), (what, "value", float(dv.max()), int(np.argmax(dv > tol)))
    if ref_arg is not None:
        inf = np.isinf(np.asarray(ref_arg).reshape(-1))
        assert (v[inf] == np.sign(np.asarray(ref_arg).reshape(-1)[inf])).all(), (what, "tanh of an infinite argument is not +-1")


# ---------------------------------------------------------------- forward jobs in a fresh process

CHILD = """import sys, numpy as np
sys.path.insert(0, %r)
from ataxxzero_amd import link, model
jobs = np.load(sys.argv[1], allow_pickle=True).item()
out, nets = {}, {}
for name, (weights, lb, mask, dtype, sym) in sorted(jobs.items()):
    if weights not in nets:
        nets[weights] = link.Net(*model.load_model(weights))
    net = nets[weights]
    p, v = (net.forward_sym if sym else net.forward)(lb, int(mask), int(dtype))
    out[name + '_p'], out[name + '_v'] = p, v
for net in nets.values():
    net.close()
np.savez(sys.argv[2], **out)
"""


def run_forward_jobs(jobs, env, tmp_path, timeout=600):
    """jobs: {name: (weights file, leaf boards, mask, dtype, sym)}.  Runs them in ONE fresh python process under the extra
    environment `env` (AZH_TOWER and AZH_TOWER_BOARDS are read once per process) -> {name + "_p" / "_v": array}"""
    job_file, out = str(tmp_path / "jobs.npy"), str(tmp_path / "out.npz")
    np.save(job_file, jobs, allow_pickle=True)
    script = str(tmp_path / "child.py")
    with open(script, "w") as f:
        f.write(CHILD % ROOT)
    res = subprocess.run([sys.executable, script, job_file, out], env=dict(os.environ, **env), capture_output=True, timeout=timeout)
    assert res.returncode == 0, res.stdout.decode()[-2000:] + res.stderr.decode()[-2000:]
    return np.load(out)
