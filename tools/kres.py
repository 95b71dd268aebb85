#!/usr/bin/env python3
"""register / scratch / LDS use of every kernel of one translation unit (hipcc -Rpass-analysis=kernel-resource-usage;
the compile and the parser are the kernel-resource tests': tests/kres_util.py):
    python tools/kres.py part_hash_inst.hip -DBTLBF_PART_H=4 [filter-substring]"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from kres_util import compile_remarks, parse_remarks  # noqa: E402

flags = [a for a in sys.argv[2:] if a.startswith("-")]
filt = [a for a in sys.argv[2:] if not a.startswith("-")]
with tempfile.TemporaryDirectory() as tmp:
    rc, err = compile_remarks(sys.argv[1], os.path.join(tmp, "kres.o"), flags)
if rc:
    print(err[-3000:])
for name, row in parse_remarks(err).items():
    if all(f in name for f in filt):
        print("%-90s vgpr %3d  scratch %4d  sgpr %3d  lds %6d" % (name[:90], row.get("vgpr", -1), row.get("scratch", -1),
                                                                   row.get("sgpr", -1), row.get("lds", -1)))
sys.exit(rc)
