"""adypt_hip --by-vertices / --recompute-normals where the command line ends before a device is asked for: a pose that tears a shared vertex (exit 1,
found while the inputs are loaded) and the two options without what they need (exit 2).  The cases are tests/test_gpu_mesh_cli.py's.  No GPU."""
from tests.test_gpu_mesh_cli import check_refusals, pose_of


def test_refusals_end_before_a_device_is_asked_for(scene_cache, tmp_path):
    check_refusals(pose_of(scene_cache), tmp_path)
