"""The fill-blend tests against the debug build with bounds-checked indexing (tools/build_variant.sh bounds: the new sites of vs_fill.hip -- the
blend kernel's tap reads 523, its read-back of pass 1's value 524 and its store 525, the channel sums' dword reads 526 and sample reads 527).
A representative subset of the blend modules runs in a child pytest with VS_AMD_LIB pointing at variants/libvs_amd_bounds.so, set up the way
tests/test_bounds_build_gpu.py sets up its children: every result must still be bit-identical (the checks change no arithmetic) and after
every test the bounds record must be clean (tests/conftest.py::_bounds_record_stays_clean)."""
import pytest

from _bounds_child import bounds_lib, child_pytest, child_python

pytestmark = pytest.mark.gpu


def test_the_bounds_build_carries_the_blend_kernels(bounds_lib):
    code = ("from video_stabilizer_amd import capi\n"
            "import numpy as np\n"
            "src = np.arange(2 * 9 * 8 * 3, dtype=np.uint8).reshape(2, 9, 8, 3)\n"
            "sums = capi.channel_sums_batch(src)\n"
            "assert sums.tolist() == src.astype(np.uint64).sum(axis=(1, 2)).tolist()\n"
            "t = capi.Transform.of(0, 0, 2, 1)\n"
            "capi.bgr_image_warp_fill_blend_batch(src, [[0, 1]], [[t, capi.Transform.of()]], sums, 2, 1)\n"
            "print('clean', capi.debug_bounds_check())\n")
    out = child_python(code, bounds_lib)
    assert "clean (0, '')" in out.stdout


def test_the_blend_modules_pass_on_the_bounds_build_with_a_clean_record(bounds_lib):
    """the hostile module first -- NaN, singular and saturating maps are what an unchecked gather would go wrong on -- then the sums, the kernel
    against the rule at the small and the multi-block sizes, and the engine's routes; without the allocation-failure walks, the app test, the long
    chunked clips and the 1080p frame (whose kernels and indices the others run as well)"""
    # (every fresh device allocation of these runs starts filled with 0xA5: nothing compared against the oracle may depend on it)
    mods = ["tests/test_fill_blend_hostile_gpu.py", "tests/test_fill_blend_gpu.py"]
    expr = ("not allocation_failure and not video_test and not chunked and not fresh_allocations and not 1080p and not engine_model "
            "and not deblur_and_denoise and not second_group")
    child_pytest(mods, expr, bounds_lib, 1200, VS_TEST_POISON_ALLOC="165", VS_TEST_HOOKS="1")
