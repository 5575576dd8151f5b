"""Device checks that need a process of their own, and the pytest side that reads their verdicts.

A SampleStore writes torch's tensors on torch's streams, so torch's HIP runtime must be mapped before the library is loaded
(link.require_torch_runtime); in a pytest process that has run other device tests it is the other way round.  A checks module
(tests/*_gpu_checks.py) therefore lists its checks in CHECKS and ends in `main(CHECKS)`: `python -m tests.<x>_gpu_checks OUT.json
[check names...]` runs them and writes {name: "ok" | traceback} to OUT.json.  The test module runs that once, in a fresh child
process (verdicts_of), and each of its tests reads one verdict (passed).  Importing this touches neither torch nor a device."""
import json
import os
import subprocess
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reads_as_device_error(text):
    """A traceback after which nothing more may run on this GPU: a faulted card is not used again."""
    t = text.lower()
    return ("hip" in t and "failed at" in t) or "illegal memory access" in t or "hip error" in t


def one_hip_runtime():
    from ataxxzero_amd import link
    link.require_gpu()
    link.require_torch_runtime()


def run(checks, path, only=(), extra=None, prepare=one_hip_runtime):
    """Runs, in order, the checks whose names are in `only` (empty: all of them) and writes {name: "ok" | traceback}, on top of
    `extra`, to `path` after every check and at the end; after a check that ends in a device error nothing more is run."""
    prepare()
    results = dict(extra or {})

    def write():
        with open(path, "w") as f:
            json.dump(results, f, indent=1)

    for check in checks:
        if only and check.__name__ not in only:
            continue
        try:
            check()
            results[check.__name__] = "ok"
        except Exception:
            results[check.__name__] = traceback.format_exc()
        write()
        if reads_as_device_error(results[check.__name__]):
            break
    write()
    return results


def main(checks, **kw):
    """The command line of a checks module: OUT.json [check names...]"""
    run(checks, sys.argv[1], sys.argv[2:], **kw)


# ---------------------------------------------------------------- the pytest side

def verdicts_of(module, path, timeout=600, echo=False):
    """`python -m <module> <path>` from the repository root in a fresh child process -> the verdicts it wrote"""
    res = subprocess.run([sys.executable, "-m", module, path], cwd=ROOT, capture_output=True, timeout=timeout)
    assert res.returncode == 0 and os.path.exists(path), (res.stdout.decode()[-2000:], res.stderr.decode()[-4000:])
    if echo:
        print(res.stdout.decode()[-2000:])
    with open(path) as f:
        return json.load(f)


def passed(verdicts, name):
    assert name in verdicts, "not run: an earlier check ended in a device error (%s)" % ", ".join(verdicts)
    assert verdicts[name] == "ok", "\n" + verdicts[name]
