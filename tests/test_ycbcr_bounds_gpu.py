"""The YCbCr tests against the debug build with bounds-checked indexing (tools/build_variant.sh bounds: vs_ycbcr.hip's row, column and frame
offsets go through VS_IDX, sites 602-615).  The ycbcr modules run in a child pytest with VS_AMD_LIB pointing at variants/libvs_amd_bounds.so, set
up the way tests/test_lens_bounds_gpu.py sets up its children: every result must still be bit-identical (the checks change no arithmetic)
and after every test the bounds record must be clean (tests/conftest.py::_bounds_record_stays_clean)."""
import pytest

from _bounds_child import bounds_lib, child_pytest, child_python

pytestmark = pytest.mark.gpu


def test_the_bounds_build_carries_the_ycbcr_record(bounds_lib):
    code = ("from video_stabilizer_amd import capi\n"
            "import numpy as np\n"
            "y = np.arange(2 * 5 * 8, dtype=np.uint8).reshape(2, 5, 8)\n"
            "c = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)\n"
            "bgr = capi.ycbcr_to_bgr_batch(y, c, c)\n"
            "capi.bgr_to_ycbcr_batch(bgr, interleaved='nv12')\n"
            "print('clean', capi.debug_bounds_check())\n")
    out = child_python(code, bounds_lib)
    assert "clean (0, '')" in out.stdout


def test_the_ycbcr_modules_pass_on_the_bounds_build_with_a_clean_record(bounds_lib):
    """the hostile module first -- odd frames whose edge cells clamp are what an unchecked offset would go wrong on -- then the kernel-level grid
    and the stabilizer's wrapper, without the allocation-failure walks, the 65 537-frame case and the tests that start children of their
    own; the CPU module rides along"""
    # (every fresh device allocation of these runs starts filled with 0xA5: nothing compared against the restatement may depend on it)
    mods = ["tests/test_ycbcr_hostile_gpu.py", "tests/test_ycbcr_gpu.py", "tests/test_ycbcr_stab_gpu.py", "tests/test_ycbcr_cpu.py"]
    expr = "not allocation_failure and not fresh_allocations and not more_frames_than_a_grid"
    child_pytest(mods, expr, bounds_lib, 1200, VS_TEST_POISON_ALLOC="165", VS_TEST_HOOKS="1")
