#!/usr/bin/env python3
"""Copy the reference's widowGo1 URDF (legged_gym/resources/robots/widowGo1/urdf/widowGo1.urdf) to tests/golden/widowGo1.urdf: the
fixture tests/test_urdf_asset.py and tests/test_gpu_urdf_asset.py load through wbc_asset_load_urdf. Only the XML is copied; the
loader never opens the meshes it names. The edited variants the tests need are made from this file at run time.

    python tools/make_golden_urdf.py REFERENCE_ROOT
"""
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REL = os.path.join("legged_gym", "resources", "robots", "widowGo1", "urdf", "widowGo1.urdf")

if len(sys.argv) != 2:
    sys.exit(__doc__)
src = os.path.join(sys.argv[1], REL)
dst = os.path.join(HERE, "..", "tests", "golden", "widowGo1.urdf")
shutil.copyfile(src, dst)
print("wrote", os.path.normpath(dst), os.path.getsize(dst), "bytes")
