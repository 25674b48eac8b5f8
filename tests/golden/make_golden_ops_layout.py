"""Regenerates tests/golden/ops_layout.json: the byte offset of every field of the reference's `struct OPS_` (src/ops.h) and its
size, as the C compiler lays it out.  tests/test_abi.py holds include/gcge_ops.h to it.
Run where a reference tree is at hand:  python tests/golden/make_golden_ops_layout.py <reference tree>"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from test_abi import layout  # noqa: E402

if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "src", "ops.h")):
    sys.exit("usage: make_golden_ops_layout.py <reference tree with src/ops.h>")
ref = sys.argv[1]
offsets, size = layout("ops.h", [os.path.join(ref, "src"), os.path.join(ref, "app")])
with open(os.path.join(HERE, "ops_layout.json"), "w") as f:
    json.dump({"struct": "OPS_", "header": "src/ops.h", "offsets": offsets, "sizeof": size}, f, indent=0)
print("struct OPS_: %d fields, sizeof %d" % (len(offsets), size))
