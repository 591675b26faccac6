"""The CPU side of profiles/walk_rows_tests.md: per scene of tests/walk_rows_scenes.py, the distance of the two fp32 references
from the float64 twin in units of 6e-8 * walk_unit, the floor they ask for between them (tests/gpu_util.py: WALK_ROW_FLOOR is
four times the largest, rounded up to a power of two), and the share of live components the rule then holds to three digits.
No device is involved.  Usage: python tools/walk_rows_md.py > table.md"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import gpu_util as G  # noqa: E402
import walk_rows_scenes as WS  # noqa: E402
from oracle import oracle  # noqa: E402

oracle.build()
print("| scene | live | oracle q50 / q99 / max | restated walk q50 / q99 / max | floor asked | held to 3 digits |")
print("|---|---|---|---|---|---|")
worst = (0.0, None)
for name in WS.NAMES:
    ref = WS.reference(oracle, name)
    so = G.walk_row_stats(ref["og"], ref["og"], ref["g64"])
    sa = G.walk_row_stats(ref["alt"], ref["og"], ref["g64"])
    asked = WS.floor_asked(G, ref)
    worst = max(worst, (asked, name))
    f = lambda q: " / ".join("%.2f" % x for x in q)
    print("| `%s` | %d | %s | %s | %.2f | %.3f |" % (name, so["live"], f(so["oracle_err_units_q50_q99_max"]),
                                                   f(sa["hip_err_units_q50_q99_max"]), asked, sa["held_3_digits"]))
print()
print("largest floor asked: %.2f on `%s`; WALK_ROW_FLOOR = %g" % (worst[0], worst[1], G.WALK_ROW_FLOOR))
