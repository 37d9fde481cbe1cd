"""Worker for test_gpu_parity.py::test_render_multi_rccl_path_on_one_device (fresh process: librccl must be the one that belongs to
the HIP runtime libjade_hip.so uses; a test process where torch was imported first already holds torch's own librccl.so.1, bound
to torch's bundled HIP runtime, and jade's dlopen of that soname would get it)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import B, config_scene, counters  # noqa: E402

assert os.environ.get("JADE_FORCE_RCCL") == "1"
hip = B.hip()
hs, cfg = config_scene("tinyjade")
p = B.params_from_config(cfg, spp=3)
p.width, p.height = 40, 30
with hip.scene(hs) as s0:
    full, full_b, st_full = s0.render(p)
    rgb, bgr, st = B.render_multi(hip, [s0], p)
assert np.array_equal(rgb.view(np.uint32), full.view(np.uint32)) and np.array_equal(bgr, full_b)
assert counters(st) == counters(st_full)
print("rccl ok")
