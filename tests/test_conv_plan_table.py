"""CPU: the conv launch planner answers what tests/golden/conv_plan_table.npz recorded, row by row.

The table (tests/golden/make_conv_plan_table.py) holds, over 67,284 geometries, the plan name, the workspace bytes, the
channel-blocked-input acceptance and the fused-GroupNorm-statistics answer of the four host queries.  The sweep is
re-run here from the same generator and compared row by row; the recorded name list must still be the 52 default plan
names, so the grid cannot be shrunk into agreement.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from image_compression_2_amd import _native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "conv_plan_table.npz")

_TILES = ["igemm_128x128", "igemm_128x128_splitk", "igemm_128x256", "igemm_256x256", "igemm_32x256",
          "igemm_32x256_splitk", "igemm_64x256"]
_PLAIN = ([f"hconv_{ci}_{co}" for ci in (32, 64, 96) for co in (32, 64)] +
          ["hg4_o128_w16_s4", "hg4_o128_w32_p2", "hg4_o192_w16_s4", "hg4_o64_w16_s4", "hg4_o64_w32_p3", "hg4_o96_w32_p2"] +
          ["igemm8_og1", "igemm8_og2", "igemm8_og2+og1", "igemm8_og2_splitk", "igemm8_og2_tail"] + _TILES + ["torgb"])
PLAN_NAMES = sorted(_PLAIN + [s + "_f16" for s in _PLAIN] + ["igemm_f32_128x128", "igemm_f32_128x128_splitk"])


@pytest.fixture(scope="module")
def swept(tmp_path_factory):
    """The sweep with the development knobs off: in this process, or in a child without the IC2_* variables when
    this one runs under IC2_DEV=1."""
    from conftest import golden_script
    gen = golden_script("make_conv_plan_table")
    if not nv.query("ic2_dev_mode"):
        return gen.sweep()
    out = str(tmp_path_factory.mktemp("plan") / "table.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("IC2_")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_conv_plan_table.py"), "--out", out],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    t = dict(np.load(out))
    t["geom"] = gen.grid().astype(np.int32)
    return t


def test_recorded_table_covers_every_default_plan_name():
    rec = np.load(TABLE)
    assert len(PLAN_NAMES) == 52
    assert sorted(rec["names"].tolist()) == PLAN_NAMES
    assert sorted(set(rec["name_idx"].tolist())) == list(range(52)), "a recorded name no row uses"
    assert len(rec["name_idx"]) == 67284
    assert int((rec["ws_bytes"] > 0).sum()) == 23363
    assert int((rec["nhwc16"] == 1).sum()) == 2724
    assert int((rec["gn_fuses"] == 1).sum()) == 190


def test_planner_matches_recorded_table(swept):
    from conftest import golden_script
    cols = golden_script("make_conv_plan_table").COLUMNS
    rec = np.load(TABLE)
    geom = swept["geom"]
    assert len(geom) == len(rec["name_idx"]), "the generator's grid is not the recorded one"
    old_names, new_names = rec["names"][rec["name_idx"]], swept["names"][swept["name_idx"]]
    bad = np.zeros(len(geom), dtype=bool)
    for key in ("ws_bytes", "nhwc16", "gn_fuses"):
        bad |= rec[key] != swept[key]
    bad |= old_names != new_names
    rows = np.flatnonzero(bad)
    report = []
    for r in rows[:8]:
        g = ", ".join(f"{c}={v}" for c, v in zip(cols, geom[r].tolist()))
        report.append(f"row {r} ({g}): plan {old_names[r]} -> {new_names[r]}, ws_bytes {rec['ws_bytes'][r]} -> "
                      f"{swept['ws_bytes'][r]}, nhwc16 {rec['nhwc16'][r]} -> {swept['nhwc16'][r]}, gn_fuses "
                      f"{rec['gn_fuses'][r]} -> {swept['gn_fuses'][r]}")
    assert len(rows) == 0, f"{len(rows)} of {len(geom)} rows differ (recorded -> now):\n" + "\n".join(report)

