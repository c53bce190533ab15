"""CPU: the Winograd launch plan (dispatch.hip: wino_plan, asked through sf_debug_wino_plan — host arithmetic, no GPU) decides what the
parent commit launched.  tests/golden/wino_plan_parent.json holds, per case, the conv_wino5_kernel launches of the commit named in it:
`traced` rows are the instantiation names (they carry the form and the block height) and grid sizes of a kernel trace of that case on the
MI355X, `derived` rows follow by hand from the inequalities of that commit's launcher (the fixture says how).  The cases: every layer of
test_gpu_wino_split.py (_CASES under SF_WINO_SPLIT_WGS unset / 0 / 1, _WIDE under SF_WINO_CAT_WIDE unset / 0), the _WINO layers of
test_gpu_conv_random.py, the gates launches of 32 x 50x50 and 2 x 200x200 latents, a single 200x200 frame with 64 / 128 output channels,
both block sizes forced (SF_WINO_SMALL_WGS = 0 / 1000000000), a group the rule of the groups refuses, and two single launches that only the
exact tests of the block decode refuse (one by a product >= 2^32, one by the grid size alone)."""
import json
import os
import subprocess
import sys

import pytest

from util import GOLD, wino_plan

_FIX = json.load(open(os.path.join(GOLD, "wino_plan_parent.json")))
_ROWS = _FIX["rows"]
_LIVE = ("SF_WINO_SPLIT_WGS", "SF_WINO_CAT_WIDE")      # re-read at every plan: set in this process; every other switch needs a fresh one


def _plan(row):
    return wino_plan(epi=row.get("epi", 0), nprob=row.get("nprob", 1), flags=row.get("flags", 0), **row["layer"])


def _check(row, plan):
    assert plan["takes"], row["id"]
    want = row["launches"]
    if want is None:      # not one launch of the kernel: a group then runs one by one, a single problem is refused; nothing is launched
        assert plan["segs"] == [], (row["id"], plan)
        return
    assert plan["form"] == want[0]["form"], (row["id"], plan)
    assert [(th, wgs) for th, _, _, wgs in plan["segs"]] == [(s["block_rows"], s["workgroups"]) for s in want], (row["id"], plan, want)
    # the windows of tile rows: together the image, the first one whole 32-tile blocks where there are two (plain / concatenated forms)
    if plan["form"] != 3:
        ty = ((row["layer"]["H"] << row["layer"].get("in_up", 0)) + 1) // 2
        rows = [(r0, n) for _, r0, n, _ in plan["segs"]]
        assert rows == ([(0, ty)] if len(rows) == 1 else [(0, ty // 4 * 4), (ty // 4 * 4, ty % 4)]), (row["id"], plan)


def test_fixture_names_its_source():
    assert len(_FIX["source"]["commit"]) == 40 and {r["origin"] for r in _ROWS} == {"traced", "derived"}
    assert len({r["id"] for r in _ROWS}) == len(_ROWS)


@pytest.mark.parametrize("row", [r for r in _ROWS if set(r.get("env", {})) <= set(_LIVE)], ids=lambda r: r["id"])
def test_plan_is_what_the_parent_launched(row):
    was = {k: os.environ.get(k) for k in _LIVE}
    try:
        for k in _LIVE:
            os.environ.pop(k, None)
        os.environ.update(row.get("env", {}))
        _check(row, _plan(row))
    finally:
        for k, v in was.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("value", ["0", "1000000000"])
def test_plan_under_a_forced_block_size(value):
    """SF_WINO_SMALL_WGS is read once per process: the rows that set it are planned by a child"""
    rows = [r for r in _ROWS if r.get("env") == {"SF_WINO_SMALL_WGS": value}]
    assert rows
    env = {k: v for k, v in os.environ.items() if k not in _LIVE}
    env["SF_WINO_SMALL_WGS"] = value
    code = ("import json, sys; sys.path.insert(0, %r); import test_wino_plan as t; "
            "print(json.dumps([t._plan(r) for r in t._ROWS if r.get('env') == {'SF_WINO_SMALL_WGS': %r}]))" % (os.path.dirname(os.path.abspath(__file__)), value))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plans = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(plans) == len(rows)
    for row, plan in zip(rows, plans):
        plan["segs"] = [tuple(s) for s in plan["segs"]]
        _check(row, plan)
