"""Children of the bounds-build tests (tests/test_bounds_build_gpu.py and the test_*_bounds_gpu.py modules): the debug build with
bounds-checked indexing (tools/build_variant.sh bounds -> variants/libvs_amd_bounds.so), and child processes that load it in place of the
regular library (VS_AMD_LIB) and have tests/conftest.py check the bounds record after every test (VS_BOUNDS_BUILD=1).

Test infrastructure only.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "video_stabilizer_amd", "variants", "libvs_amd_bounds.so")


@pytest.fixture(scope="module")
def bounds_lib(gpu_vs):
    # (built on demand, and again whenever a source of the library is newer than it: a stale variant would test yesterday's kernels)
    csrc = os.path.join(ROOT, "video_stabilizer_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".hpp", ".inc", ".cpp"))] + [os.path.join(ROOT, "include", "vs_amd.h")]
    if not os.path.exists(LIB) or max(os.path.getmtime(f) for f in srcs) > os.path.getmtime(LIB):
        subprocess.check_call(["bash", os.path.join(ROOT, "tools", "build_variant.sh"), "bounds"])
    assert os.path.exists(LIB)
    return LIB


def _env(lib, extra):
    """this process's environment with the bounds build in place of the library; extra: further variables, None takes one out"""
    env = dict(os.environ, VS_AMD_LIB=lib, VS_BOUNDS_BUILD="1")
    for k, v in extra.items():
        if v is None:
            env.pop(k, None)
        else:
            env[k] = v
    return env


def child_python(code, lib, **env):
    """`code` in a python of its own with the repository on its path -> the finished process, its return code asserted 0"""
    out = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n" % ROOT + code], env=_env(lib, env), capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return out


def child_pytest(mods, expr, lib, timeout, **env):
    """the test modules `mods` in a pytest of its own, -k expr (None: all of them), stopping at the first failure: it must pass"""
    cmd = [sys.executable, "-m", "pytest", *mods, "-x", "-q", "-p", "no:cacheprovider"] + (["-k", expr] if expr else [])
    out = subprocess.run(cmd, cwd=ROOT, env=_env(lib, env), capture_output=True, text=True, timeout=timeout)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "failed" not in out.stdout, tail
