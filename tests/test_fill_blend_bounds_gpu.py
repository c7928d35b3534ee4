"""The fill-blend tests against the debug build with bounds-checked indexing (tools/build_variant.sh bounds: the new sites of vs_fill.hip -- the
blend kernel's tap reads 523, its read-back of pass 1's value 524 and its store 525, the channel sums' dword reads 526 and sample reads 527).
A representative subset of the blend modules runs in a child pytest with VS_AMD_LIB pointing at variants/libvs_amd_bounds.so, set up the way
tests/test_bounds_build_gpu.py sets up its children: every result must still be bit-identical (the checks change no arithmetic) and after
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


def test_the_bounds_build_carries_the_blend_kernels(bounds_lib):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from video_stabilizer_amd import capi\n"
            "import numpy as np\n"
            "src = np.arange(2 * 9 * 8 * 3, dtype=np.uint8).reshape(2, 9, 8, 3)\n"
            "sums = capi.channel_sums_batch(src)\n"
            "assert sums.tolist() == src.astype(np.uint64).sum(axis=(1, 2)).tolist()\n"
            "t = capi.Transform.of(0, 0, 2, 1)\n"
            "capi.bgr_image_warp_fill_blend_batch(src, [[0, 1]], [[t, capi.Transform.of()]], sums, 2, 1)\n"
            "print('clean', capi.debug_bounds_check())\n" % ROOT)
    env = dict(os.environ, VS_AMD_LIB=bounds_lib, VS_BOUNDS_BUILD="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "clean (0, '')" in out.stdout


def test_the_blend_modules_pass_on_the_bounds_build_with_a_clean_record(bounds_lib):
    """the hostile module first -- NaN, singular and saturating maps are what an unchecked gather would go wrong on -- then the sums, the kernel
    against the rule at the small and the multi-block sizes, and the engine's routes; without the allocation-failure walks, the app test, the long
    chunked clips and the 1080p frame (whose kernels and indices the others run as well)"""
    # (every fresh device allocation of these runs starts filled with 0xA5: nothing compared against the oracle may depend on it)
    env = dict(os.environ, VS_AMD_LIB=bounds_lib, VS_BOUNDS_BUILD="1", VS_TEST_POISON_ALLOC="165", VS_TEST_HOOKS="1")
    mods = ["tests/test_fill_blend_hostile_gpu.py", "tests/test_fill_blend_gpu.py"]
    expr = ("not allocation_failure and not video_test and not chunked and not fresh_allocations and not 1080p and not engine_model "
            "and not deblur_and_denoise and not second_group")
    cmd = [sys.executable, "-m", "pytest", *mods, "-x", "-q", "-p", "no:cacheprovider", "-k", expr]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "failed" not in out.stdout, tail
