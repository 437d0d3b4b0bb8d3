"""The device-side headers the batch objects share, read as text: device functions only, nothing of the depth path."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "mono_lidar_depth_amd" / "csrc"


def _holds_no_kernel_and_is_unknown_to_the_depth_path(name, public_header=False):
    text = (CSRC / "batch" / f"{name}.h").read_text()
    assert "__global__" not in text
    for inc in re.findall(r'#include\s+"([^"]+)"', text):
        path = (CSRC / "batch" / inc).resolve()
        assert path.parent == (CSRC / "batch").resolve() or (public_header and path == (ROOT / "include" / "mld.h").resolve()), inc
    for path in CSRC.iterdir():
        if path.is_file() and path.name != "Makefile":
            assert name not in path.read_text(), path.name


def test_the_shared_device_header_holds_no_kernel_and_nothing_of_the_depth_path():
    """batch/mld_batch_device.h has no kernel, its quoted includes stay inside batch/, and no file directly in csrc/
    (the depth path, the Makefile aside) names it."""
    _holds_no_kernel_and_is_unknown_to_the_depth_path("mld_batch_device")


def test_the_depth_path_header_is_held_to_the_same():
    """batch/mld_depth_path.h likewise; its quoted includes may also be the public header."""
    _holds_no_kernel_and_is_unknown_to_the_depth_path("mld_depth_path", public_header=True)


def test_the_depth_path_header_restates_and_does_not_reach_into_the_depth_path():
    """batch/mld_depth_path.h includes mld_batch_device.h and the public header and nothing else of the project, names
    neither of the depth path's internal headers, has no inline assembly, and describes its users by role: the units that
    no file outside their directory may name are not named."""
    text = (CSRC / "batch" / "mld_depth_path.h").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["mld_batch_device.h", "../../../include/mld.h"]
    assert "mld_device.h" not in text and "mld_diag.h" not in text
    assert "asm" not in re.sub(r"//.*", "", text)
    for unit in ("mld_coverage", "mld_depth_image", "mld_region"):
        assert unit not in text, unit
    assert re.search(r"^SRC\s*:=.*batch/mld_batch_device\.h batch/mld_depth_path\.h", (CSRC / "Makefile").read_text(), flags=re.M)


def test_the_batch_units_take_and_return_gpu_memory_through_the_object_header_only():
    """Under the subdirectories of csrc/ only batch/mld_batch_object.h frees (and no unit has a free_own left), no unit
    allocates by itself, and the shared types of that header have no release() to be called by hand."""
    header = CSRC / "batch" / "mld_batch_object.h"
    for path in CSRC.rglob("*"):
        if not path.is_file() or path.parent == CSRC or path == header:
            continue
        text = path.read_text()
        for word in ("hipFree", "hipHostFree", "free_own"):
            assert word not in text, (path.name, word)
        assert "hipMalloc(" not in text, path.name
    assert not re.search(r"\brelease\s*\(", header.read_text())


def test_the_functions_of_the_depth_path_header_exist_once_among_the_batch_units():
    """What the header took over is defined nowhere else under csrc/ outside the depth path's own files."""
    names = ("prefix_count", "uniform", "reduce_best", "wave_sum", "wave_max", "vsub", "vadd", "vscale", "vdivs", "vdot", "vsqnorm",
             "vnorm", "vnormalized", "vcross", "smallest_eigvec3", "plane_through", "viewing_ray", "intersect", "apply_thresholds",
             "finish_main", "window_bounds", "far_from_plane", "mask_bit", "list_point", "max_spanning_triangle", "list_minmax_z",
             "hist_segment", "gather_window", "inverse3", "window_cells", "window_span", "build_calib", "main_path", "read_feature",
             "store_record", "feature_table_fault", "feature_sign_fault", "feature_capacity_fault", "feature_array_fault",
             "feature_alignment_fault", "feature_grid")
    shared = {"mld_batch_device.h", "mld_depth_path.h"}
    for path in CSRC.rglob("*"):
        if not path.is_file() or path.parent == CSRC:
            continue
        code = re.sub(r"//.*", "", path.read_text())
        for name in names:
            defs = re.findall(r"^(?!\s*return\b)[\w \t:<>&*]*[\w>&*]\s+" + name + r"\([^;{]*\)\s*\{", code, flags=re.M)
            if path.name in shared:
                continue
            # (the coverage maps fill their own calibration: same name, their own struct)
            if name == "build_calib" and path.name == "mld_coverage_maps.hip":
                continue
            # (the cooperative route of the depth images keeps its gather: profiles/depth_path_header.md)
            if name == "gather_window" and path.name == "mld_depth_images.hip":
                assert len(defs) == 1 and "profiles/depth_path_header.md" in path.read_text()
                continue
            assert defs == [], (path.name, name)
    both = "".join(re.sub(r"//.*", "", (CSRC / "batch" / h).read_text()) for h in shared)
    for name in names:
        n = len(re.findall(r"^(?:template[^\n]*\n)?[\w \t:<>&*]*[\w>&*]\s+" + name + r"\([^;{]*\)\s*\{", both, flags=re.M))
        assert n == (2 if name in ("wave_sum", "mask_bit") else 1), (name, n)


def test_the_feature_traces_run_the_main_path_of_the_header():
    """The sequence of calls behind the neighbour search exists once among the batch units: the trace names main_path and
    none of the functions it strings together."""
    code = re.sub(r"//.*", "", (CSRC / "traces" / "mld_feature_traces.hip").read_text())
    assert "main_path(" in code
    for name in ("hist_segment(", "max_spanning_triangle(", "list_minmax_z(", "finish_main("):
        assert name not in code, name
