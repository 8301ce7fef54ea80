"""Record cimq_module_wide_plan of every descriptor row of tests/golden/wide_parent_table.json, as answered by the
library ``CIMQ_LIB_PATH`` names (else this tree's): the fixture tests/test_pool_host.py holds the wide plans to.

    CIMQ_LIB_PATH=<another revision's libcimq.so> python tools/record_wide_plans.py tests/golden/pool_parent_plans.json
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import cim_quantization_amd._lib as L  # noqa: E402
from test_pool_host import _plan_rows  # noqa: E402

if __name__ == "__main__":
    _, plans = _plan_rows(L.load())
    with open(sys.argv[1], "w") as f:
        f.write('{"columns": ["rc", "ok", "chunks", "groups", "tiles"],\n "plans": [\n')
        f.write(",\n".join("  " + json.dumps(p) for p in plans))
        f.write("\n ]}\n")
    print(f"{len(plans)} plans from {L.LIB_PATH}")
