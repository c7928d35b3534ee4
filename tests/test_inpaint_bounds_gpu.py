"""The inpaint tests against the debug build with bounds-checked indexing (tools/build_variant.sh bounds: every LDS index of the tail, every
pyramid index, the mask and the window stores of vs_inpaint.hip go through VS_IDX, sites 561-575).  The three inpaint modules run in a child pytest
with VS_AMD_LIB pointing at variants/libvs_amd_bounds.so, set up the way tests/test_bounds_build_gpu.py sets up its children: every result must
still be bit-identical (the checks change no arithmetic) and after every test the bounds record must be clean
(tests/conftest.py::_bounds_record_stays_clean)."""
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


def test_the_bounds_build_carries_the_inpaint_record(bounds_lib):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from video_stabilizer_amd import capi\n"
            "import numpy as np\n"
            "img = np.arange(2 * 5 * 8 * 3, dtype=np.uint8).reshape(2, 5, 8, 3)\n"
            "mask = (np.arange(2 * 5 * 8).reshape(2, 5, 8) & 3 != 0).astype(np.uint8)\n"
            "capi.bgr_inpaint_batch(img, mask)\n"
            "capi.bgr_fill_coverage_batch(8, 5, [[0]], [[capi.Transform.of(0, 0, 2, 1)]])\n"
            "print('clean', capi.debug_bounds_check())\n" % ROOT)
    env = dict(os.environ, VS_AMD_LIB=bounds_lib, VS_BOUNDS_BUILD="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "clean (0, '')" in out.stdout


def test_the_inpaint_modules_pass_on_the_bounds_build_with_a_clean_record(bounds_lib):
    """the kernel-level modules and the stabilizer module's shapes, without the allocation-failure walks, the app test, the child-process
    poison run and the long chunked clip (whose kernels and indices the short clips run as well), and without the hostile module's
    65537-frame batches and its child processes.  1 x 4096 in 16 bits is the point of the hostile module here: the tail's 8191 texels against
    the LDS array (sites 572-575)"""
    # (every fresh device allocation of these runs starts filled with 0xA5: nothing compared against the rule may depend on it)
    env = dict(os.environ, VS_AMD_LIB=bounds_lib, VS_BOUNDS_BUILD="1", VS_TEST_POISON_ALLOC="165", VS_TEST_HOOKS="1")
    mods = ["tests/test_inpaint_gpu.py", "tests/test_inpaint_stab_gpu.py", "tests/test_inpaint_hostile_gpu.py"]
    expr = "not allocation_failure and not video_test and not time_chunks and not fresh_allocations and not 65535_frame_line and not scratch_groups"
    cmd = [sys.executable, "-m", "pytest", *mods, "-x", "-q", "-p", "no:cacheprovider", "-k", expr]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "failed" not in out.stdout, tail
