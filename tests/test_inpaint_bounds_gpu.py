"""The inpaint tests against the debug build with bounds-checked indexing (tools/build_variant.sh bounds: every LDS index of the tail, every
pyramid index, the mask and the window stores of vs_inpaint.hip go through VS_IDX, sites 561-575).  The three inpaint modules run in a child pytest
with VS_AMD_LIB pointing at variants/libvs_amd_bounds.so, set up the way tests/test_bounds_build_gpu.py sets up its children: every result must
still be bit-identical (the checks change no arithmetic) and after every test the bounds record must be clean
(tests/conftest.py::_bounds_record_stays_clean)."""
import pytest

from _bounds_child import bounds_lib, child_pytest, child_python

pytestmark = pytest.mark.gpu


def test_the_bounds_build_carries_the_inpaint_record(bounds_lib):
    code = ("from video_stabilizer_amd import capi\n"
            "import numpy as np\n"
            "img = np.arange(2 * 5 * 8 * 3, dtype=np.uint8).reshape(2, 5, 8, 3)\n"
            "mask = (np.arange(2 * 5 * 8).reshape(2, 5, 8) & 3 != 0).astype(np.uint8)\n"
            "capi.bgr_inpaint_batch(img, mask)\n"
            "capi.bgr_fill_coverage_batch(8, 5, [[0]], [[capi.Transform.of(0, 0, 2, 1)]])\n"
            "print('clean', capi.debug_bounds_check())\n")
    out = child_python(code, bounds_lib)
    assert "clean (0, '')" in out.stdout


def test_the_inpaint_modules_pass_on_the_bounds_build_with_a_clean_record(bounds_lib):
    """the kernel-level modules and the stabilizer module's shapes, without the allocation-failure walks, the app test, the child-process
    poison run and the long chunked clip (whose kernels and indices the short clips run as well), and without the hostile module's
    65537-frame batches and its child processes.  1 x 4096 in 16 bits is the point of the hostile module here: the tail's 8191 texels against
    the LDS array (sites 572-575)"""
    # (every fresh device allocation of these runs starts filled with 0xA5: nothing compared against the rule may depend on it)
    mods = ["tests/test_inpaint_gpu.py", "tests/test_inpaint_stab_gpu.py", "tests/test_inpaint_hostile_gpu.py"]
    expr = "not allocation_failure and not video_test and not time_chunks and not fresh_allocations and not 65535_frame_line and not scratch_groups"
    child_pytest(mods, expr, bounds_lib, 1200, VS_TEST_POISON_ALLOC="165", VS_TEST_HOOKS="1")
