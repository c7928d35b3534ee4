"""The sharpen tests against the debug build with bounds-checked indexing (tools/build_variant.sh bounds: every global access of vs_sharpen.hip goes
through VS_IDX, sites 621-628).  The two kernel modules run in a child pytest with VS_AMD_LIB pointing at variants/libvs_amd_bounds.so, set up the
way tests/test_scene_bounds_gpu.py sets up its children: every result must still be bit-identical (the checks change no arithmetic) and after
every test the bounds record must be clean (tests/conftest.py::_bounds_record_stays_clean)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
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


def test_the_bounds_build_carries_the_sharpen_record(bounds_lib):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from video_stabilizer_amd import capi\n"
            "import numpy as np\n"
            "src = (np.arange(2 * 5 * 8 * 3, dtype=np.uint8).reshape(2, 5, 8, 3) * 7 %% 200) + 20\n"
            "out = capi.sharpen_batch(src, [capi.Transform.of(0, 0, 0.5, 0.5), capi.Transform.of()], 8, 5)\n"
            "print('changed', bool((out[0] != src[0]).any()), 'same', bool((out[1] == src[1]).all()), 'clean', capi.debug_bounds_check())\n" % ROOT)
    env = dict(os.environ, VS_AMD_LIB=bounds_lib, VS_BOUNDS_BUILD="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "changed True same True clean (0, '')" in out.stdout, out.stdout


def test_the_sharpen_modules_pass_on_the_bounds_build_with_a_clean_record(bounds_lib):
    """the hostile module first -- NaN, singular and saturating maps and windows inside poison are what an unchecked access would go wrong on --
    then the kernel-level one"""
    # (every fresh device allocation of these runs starts filled with 0xA5: nothing compared against the restatement may depend on it)
    env = dict(os.environ, VS_AMD_LIB=bounds_lib, VS_BOUNDS_BUILD="1", VS_TEST_POISON_ALLOC="165", VS_TEST_HOOKS="1")
    mods = ["tests/test_sharpen_hostile_gpu.py", "tests/test_sharpen_gpu.py"]
    cmd = [sys.executable, "-m", "pytest", *mods, "-x", "-q", "-p", "no:cacheprovider"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "failed" not in out.stdout, tail
