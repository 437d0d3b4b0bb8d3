"""The device-side header the batch objects share, read as text: device functions only, nothing of the depth path."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_the_shared_device_header_holds_no_kernel_and_nothing_of_the_depth_path():
    """batch/mld_batch_device.h has no kernel, its quoted includes stay inside batch/, and no file directly in csrc/
    (the depth path, the Makefile aside) names it."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    text = (csrc / "batch" / "mld_batch_device.h").read_text()
    assert "__global__" not in text
    for inc in re.findall(r'#include\s+"([^"]+)"', text):
        assert (csrc / "batch" / inc).resolve().parent == (csrc / "batch").resolve(), inc
    for path in csrc.iterdir():
        if path.is_file() and path.name != "Makefile":
            assert "mld_batch_device" not in path.read_text(), path.name
